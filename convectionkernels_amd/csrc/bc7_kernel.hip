// BC7 endpoint / partition / index search for gfx950 (MI355X), hand-written HIP.
//
// What it replaces: cvtt::Internal::BC7Computer::Pack and everything under it
// (reference ConvectionKernels_BC67.cpp:1975-2204 -> TrySinglePlane 1042-1662,
// TryDualPlane 1664-1965, CompressEndpoints* 829-938; EndpointSelector.h, EndpointRefiner.h,
// IndexSelector.h, AggregatedError.h).  Results are bit-identical to the reference's SSE2
// lanes; the arithmetic contract is kept by compiling this file with
// -ffp-contract=off and IEEE divide/sqrt, f32 denormals on.
//
// Mapping (this is not the reference's 8-blocks-per-SSE-register layout; DESIGN.md 4.1 has the measurements):
//   * one wavefront = 16 blocks = two reference "groups" of 8; lanes [0,32) and [32,64) each
//     form one group, whose two alpha-derived booleans (BC67.cpp:1069, 1072) are wave ballots.
//   * exact branch-and-bound: a rigorous lower bound on the error of ANY trial of a shape (its
//     total-least-squares residual minus the allowance for rounding, cvtt_kernel_common.h) is compared with the
//     block's best error so far; a candidate that cannot pass the reference's commit test is skipped, which leaves
//     the output bit-identical.  Whole-block bounds order and prune the four rotations of modes 4/5 and mode 6;
//     bounds of all 64 partitions (2-D projection, v_dot4 / v_dot2 masked sums) go to LDS per mode family, and the
//     partitions they leave alive get the same bound in all channels of each subset (raw integer sums, second tier).
//   * dual-plane modes 4/5: a block is owned by a lane QUAD, sub-lane = seed point; the block is held channel-major,
//     the float index selection and refiner sums are the reference's operations, the integer error comes from level
//     tables + v_perm_b32 + v_dot4_u32_u8 (evalDual, bc7_dual.h; slow indexing probes from the same tables).
//   * single-plane modes 0-3, 6, 7: work pooled over the wave.  Per round the blocks offer their cheapest-bound
//     partitions, one lane per (item, subset) runs the PCA seed search on LDS-staged pixels, then one lane per CHAIN
//     (p-bit combination x seed point, with its serial refine rounds: evalChain) evaluates it; an order-preserving
//     argmin reproduces the reference's first-minimum rule and the owning block commits by (error, position in the
//     reference's candidate order), so the evaluation order is free.
//   * BC7_RespectPunchThrough (separate instantiation): the commit rule couples the 8 blocks of a group per trial;
//     every trial's error is recorded in LDS and the rule is replayed over 8-lane ballot slices.
//   * modes 4 / 5 are packed by one lane at constant bit positions; for the other modes the quad packs the (up to 66)
//     bit fields of its block in parallel; sub-lane 0 stores the 16 bytes.
//   * large inputs: a wave that would still have many mode-7 partitions to search near the end of the grid hands those
//     blocks to a second launch (HARD instantiation, 16 waves per block) and a commit launch picks the winner.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <type_traits>
#include <stdlib.h>

#include "cvtt_device.h"

// BC7_RespectPunchThrough: refine rounds whose trial errors are kept in LDS (2 KB per round; the reference's default is 2
// rounds).  With more rounds the table of a wave lives in HBM (CvttBc7Args::ptTrial).  6 rounds of LDS held this
// instantiation at 6 workgroups per CU; 2 rounds: 10 (2.5 waves per SIMD).
constexpr int kMaxPTRefine = 2;
// half-range of the integer grid the projected points are rounded to: 12-bit coordinates summed with v_dot2_i32_i16, or
// 8-bit ones summed with v_dot4_i32_i8 (half the instructions, bounds looser by the coarser rounding)
constexpr float kBoundGrid16 = 2000.0f, kBoundLimit16 = 2040.0f;
constexpr float kBoundGrid8 = 124.0f, kBoundLimit8 = 127.0f;
// which grid the first-tier bounds of the RGBA partitions (mode 7) and of the RGB partitions (modes 0-3) use.  With the
// second tier behind them the cheaper bounds win everywhere (RGBA noise +3 %, photo-like opaque content +6 %, opaque
// noise equal); the 12-bit grid stays selectable for experiments.
#ifndef CVTT_GRID8_RGBA
#define CVTT_GRID8_RGBA true
#endif
#ifndef CVTT_GRID8_RGB
#define CVTT_GRID8_RGB true
#endif
// Waves per SIMD the register allocator must leave room for (512 VGPRs / waves).  4 since round 2: the kernel fits 8 LDS
// granules (16-bit bound table, 64 result slots), and the dual-plane search reads the block's channel-major pixels, the
// rotation's seeds and the per-block invariants from LDS where it uses them, which brought the 128-register build from
// 43 spilled registers to 33.  Measured 3 -> 4 waves: RGBA noise 630 -> 672 Mblocks/s at 4096^2, opaque noise 136 -> 150,
// smooth / photo-like / two-colour content +13 % (chain rounds are plain f32 arithmetic, which an EVEN number of resident
// waves overlaps: profiles/r02/valu_order.txt).
#ifndef CVTT_BC7_WAVES
#define CVTT_BC7_WAVES 4
#endif
// the same for the slow-indexing instantiation (Flags::Better / Ultra), whose three probes per pixel need more registers
// (4 since round 3: with the pixel loop of its dual-plane search rolled into four trips the instantiation fits 128
// registers; Flags::Better on 4096^2 RGBA noise 292 -> 306 Mblocks/s, opaque 75 -> 78)
#ifndef CVTT_BC7_WAVES_SLOW
#define CVTT_BC7_WAVES_SLOW 4
#endif
// power iterations per principal axis of the projection the first-tier bounds are taken in (tightness only, never validity)
#ifndef CVTT_EIG_ITERS
#define CVTT_EIG_ITERS 6
#endif

#include "cvtt_kernel_common.h"
#include "cvtt_launchers.h"

// candidates a block may offer per round when 1 / 2 / <=4 / <=8 blocks of the wave offer at all
#ifndef CVTT_SPEC_1
#define CVTT_SPEC_1 32
#define CVTT_SPEC_2 16
#define CVTT_SPEC_4 8
#define CVTT_SPEC_8 4
#endif
#ifndef CVTT_SPEC_16
#define CVTT_SPEC_16 2
#endif
// probe survivors a wave collects before it searches them in full (one full-search chunk holds 32 / 21 partitions)
#ifndef CVTT_FILTER_STRIKES
#define CVTT_FILTER_STRIKES 2
#endif
#ifndef CVTT_SHARP_COST4
#define CVTT_SHARP_COST4 64
#endif
#ifndef CVTT_SHARP_COST8
#define CVTT_SHARP_COST8 20
#endif
#ifndef CVTT_PEND_MIN
#define CVTT_PEND_MIN 20
#endif

// Developer-only phase profile (-DCVTT_BC7_PROFILE): wave cycles per phase, summed over waves.
#ifdef CVTT_BC7_PROFILE
__device__ unsigned long long g_bc7Prof[48];
__device__ unsigned long long g_bc7Dup[8]; // chain rounds: total, same endpoints as a lower seed point this round, seen in an earlier round of the group
// per single-plane stage (6, 7, 1, 3, 0, 2): chain batches, units searched, partitions alive when the stage starts (after
// both bound tiers), offer rounds, partitions committed as the block's new best, active chain lanes, wave-stages entered
__device__ unsigned long long g_bc7Stage[6][8];
__device__ unsigned long long g_bc7Stage2[6][8]; // spare
extern "C" int cvttmi_bc7_stage_read(unsigned long long *out)
{
    unsigned long long zero[48] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bc7Stage), sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7Stage), zero, sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out + 48, HIP_SYMBOL(g_bc7Stage2), sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7Stage2), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#define PROF_STAGE(stage, slot, n) { const unsigned long long v_ = (unsigned long long)(n); if (threadIdx.x == 0 && v_) atomicAdd(&g_bc7Stage[stage][slot], v_); }
#define PROF_STAGE_LANES(stage, slot, pred) { const unsigned long long v_ = (unsigned long long)__popcll(__ballot(pred)); if (threadIdx.x == 0 && v_) atomicAdd(&g_bc7Stage[stage][slot], v_); }
#define PROF_STAGE2(stage, slot, n) { const unsigned long long v_ = (unsigned long long)(n); if (threadIdx.x == 0 && v_) atomicAdd(&g_bc7Stage2[stage][slot], v_); }
extern "C" int cvttmi_bc7_dup_read(unsigned long long *out)
{
    unsigned long long zero[8] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bc7Dup), sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7Dup), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
// One record per wave of the encoder's launch (tools/bc7_phase_overlap.py), ten 64-bit words in the buffer that
// cvttmi_bc7_wave_trace_set names (record = workgroup index; none beyond the capacity).  Lane 0 writes every word with an
// ordinary store where it arises, so that no time stamp has to live in a register across the search:
//   0  HW_ID (wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13]) | XCC_ID << 32, from s_getreg
//   1  shader clock at the start     2..4  at PROF_MARK 6 (block loaded and bounded), 0 (dual-plane seeds done = the search starts),
//   1 (the search is over)           5, 6  begin and end of the wave's longest partition-bounds interval (PROF_MARK 2; 0: none)
//   7  shader clock at the end       8, 9  the 100 MHz wall clock (s_memrealtime) at the start and at the end
// The shader clock is compared only among the waves of one SIMD.  The caller zeroes the buffer before the encode.
__device__ unsigned long long *g_bc7WaveTrace;
__device__ u32 g_bc7WaveTraceCap;
extern "C" int cvttmi_bc7_wave_trace_set(void *deviceBuffer, uint32_t capacityRecords)
{
    unsigned long long *buf = static_cast<unsigned long long *>(deviceBuffer);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7WaveTrace), &buf, sizeof(buf)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7WaveTraceCap), &capacityRecords, sizeof(capacityRecords)) != hipSuccess) return -1;
    return 0;
}
#define PROF_REC(word, value) { if (!HARD && __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0u) { unsigned long long *const tb_ = g_bc7WaveTrace; \
    if (tb_ != nullptr && vBlock < g_bc7WaveTraceCap) tb_[(size_t)vBlock * 10u + (word)] = (value); } }
#define PROF_TRACE_DECL u32 profB2len = 0; PROF_REC(1, profT) PROF_REC(8, __builtin_amdgcn_s_memrealtime()) \
    PROF_REC(0, (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) | ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32))
#define PROF_TRACE_MARK(slot) { if ((slot) == 6) PROF_REC(2, now) if ((slot) == 0) PROF_REC(3, now) if ((slot) == 1) PROF_REC(4, now) \
    if ((slot) == 2 && (u32)(now - profT) > profB2len) { profB2len = (u32)(now - profT); PROF_REC(5, profT) PROF_REC(6, now) } }
#define PROF_TRACE PROF_REC(7, profT) PROF_REC(9, __builtin_amdgcn_s_memrealtime())
#define PROF_DECL unsigned long long profT = __builtin_readcyclecounter(); unsigned long long profAcc[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long profCnt[8] = {0, 0, 0, 0, 0, 0, 0, 0}; PROF_TRACE_DECL
#define PROF_MARK(slot) { const unsigned long long now = __builtin_readcyclecounter(); profAcc[slot] += now - profT; PROF_TRACE_MARK(slot) profT = now; }
#define PROF_FLUSH if (threadIdx.x == 0) { unsigned long long tot = 0; for (int i = 0; i < 16; i++) { atomicAdd(&g_bc7Prof[i], profAcc[i]); tot += profAcc[i]; } \
    int bucket = 63 - __builtin_clzll(tot | 1ull) - 12; bucket = bucket < 0 ? 0 : (bucket > 15 ? 15 : bucket); atomicAdd(&g_bc7Prof[16 + bucket], 1ull); \
    } { unsigned long long wsum[8]; for (int i = 0; i < 8; i++) { unsigned long long v = profCnt[i]; if (i >= 4) { for (int st = 1; st < 64; st <<= 1) v += __shfl_xor(v, st); } wsum[i] = v; } \
    if (threadIdx.x == 0) { for (int i = 0; i < 8; i++) atomicAdd(&g_bc7Prof[32 + i], wsum[i]); \
    const unsigned long long passes = profCnt[2] / 64ull; int pb = 63 - __builtin_clzll(passes | 1ull); pb = pb > 7 ? 7 : pb; atomicAdd(&g_bc7Prof[40 + pb], 1ull); } }
#define PROF_COUNT(slot, n) { profCnt[slot] += (unsigned long long)(n); }
// -DCVTT_BC7_PROFILE=2: the wave records alone.  The sums and counters above cost the kernel registers it does not have (the
// full profile build spills); the records need three scalars, so this build keeps four waves per SIMD without scratch and
// its waves line up as the default build's do.
#if CVTT_BC7_PROFILE + 0 == 2
#undef PROF_DECL
#undef PROF_MARK
#undef PROF_COUNT
#undef PROF_FLUSH
#undef PROF_STAGE
#undef PROF_STAGE2
#undef PROF_STAGE_LANES
#define PROF_DECL unsigned long long profT = __builtin_readcyclecounter(); PROF_TRACE_DECL
#define PROF_MARK(slot) { const unsigned long long now = __builtin_readcyclecounter(); PROF_TRACE_MARK(slot) profT = now; }
#define PROF_COUNT(slot, n)
#define PROF_FLUSH
#define PROF_STAGE(stage, slot, n)
#define PROF_STAGE2(stage, slot, n)
#define PROF_STAGE_LANES(stage, slot, pred)
#endif
extern "C" int cvttmi_bc7_prof_read(unsigned long long *out)
{
    unsigned long long zero[48] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bc7Prof), sizeof(zero)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7Prof), zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
#else
#define PROF_DECL
#define PROF_MARK(slot)
#define PROF_COUNT(slot, n)
#define PROF_FLUSH
#define PROF_TRACE
#define PROF_STAGE(stage, slot, n)
#define PROF_STAGE2(stage, slot, n)
#define PROF_STAGE_LANES(stage, slot, pred)
#endif

// Developer-only bound dump (-DCVTT_BC7_BOUND_DUMP, lib/variants/libcvtt_mi355x_bounddump.so): every value the search compares
// with a block's best error in order to drop a candidate is appended to a device buffer as one 48-byte record, where it is
// formed and where it is read back and compared (tests/test_bc7_bound_soundness.py holds each one to the exact bound in
// float64 and to the error the reference reaches for the candidate).  Twelve words per record:
//   0  block index
//   1  tier | kind << 8 | (second launch) << 16
//        tier: 0 whole block (mode 6), 1 rotation (modes 4 / 5), 2 first tier, 3 second tier plain (subsetBoundFull),
//              4 second tier sharp (subsetBoundSharp), 5 probe + plain bound of the rest, 6 probe + sharp bound of the rest,
//              7 the block's final error
//        kind: 0 formed (and stored), 1 formed, stored and compared, 2 read back from the table and compared,
//              3 one subset's share of a sharp bound (words 8..11: the direction d it used), 4 final error
//   2  bound set | mode << 8 | subsets << 16 | index bits the value holds for << 24  (4 = any mode of the set)
//   3  partition or rotation | subset << 8
//   4  the value as computed      5  the value as the table gives it back (fabs of the upper 16 bits; the value itself where
//   6  the best error compared with   7  1 = dropped                                                    it is kept in a register)
//   8..11  per site: the static alpha error, the probed subset's error and the bound of the rest, d, ...
// The counter advances with an ordinary atomicAdd; records past the capacity are counted and not written.
#ifdef CVTT_BC7_BOUND_DUMP
__device__ u32 *g_bc7BoundBuf;
__device__ u32 g_bc7BoundCap;
__device__ u32 g_bc7BoundCount;
extern "C" int cvttmi_bc7_bound_dump_set(void *deviceBuffer, uint32_t capacityRecords)
{
    const uint32_t zero = 0;
    u32 *buf = static_cast<u32 *>(deviceBuffer);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7BoundBuf), &buf, sizeof(buf)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7BoundCap), &capacityRecords, sizeof(capacityRecords)) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_bc7BoundCount), &zero, sizeof(zero)) != hipSuccess) return -1;
    return 0;
}
extern "C" int cvttmi_bc7_bound_dump_count(uint32_t *out)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bc7BoundCount), sizeof(*out)) == hipSuccess ? 0 : -1;
}
enum : u32 { BD_WHOLE6 = 0, BD_ROT = 1, BD_TIER1 = 2, BD_FULL = 3, BD_SHARP = 4, BD_PROBE_FULL = 5, BD_PROBE_SHARP = 6, BD_FINAL = 7 };
enum : u32 { BD_FORM = 0, BD_FORM_CMP = 1, BD_RELOAD = 2, BD_SUBSET = 3, BD_END = 4 };
__device__ __noinline__ void boundDumpEmit(u32 block, u32 w1, u32 w2, u32 w3, float computed, float stored, float err, u32 dropped,
                                           float x0, float x1, float x2, float x3)
{
    u32 *const buf = g_bc7BoundBuf;
    if (buf == nullptr)
        return;
    const u32 at = atomicAdd(&g_bc7BoundCount, 1u);
    if (at >= g_bc7BoundCap)
        return;
    u32 *r = buf + (size_t)at * 12u;
    r[0] = block;
    r[1] = w1;
    r[2] = w2;
    r[3] = w3;
    r[4] = __builtin_bit_cast(u32, computed);
    r[5] = __builtin_bit_cast(u32, stored);
    r[6] = __builtin_bit_cast(u32, err);
    r[7] = dropped;
    r[8] = __builtin_bit_cast(u32, x0);
    r[9] = __builtin_bit_cast(u32, x1);
    r[10] = __builtin_bit_cast(u32, x2);
    r[11] = __builtin_bit_cast(u32, x3);
}
#define BOUND_DUMP(...) do { __VA_ARGS__; } while (0)
#else
#define BOUND_DUMP(...)
#endif

// The helpers of the search (they use the knobs and the PROF_* macros above): what the phases share and the single-plane
// chains, the dual-plane search, the partition bounds.  bc7Body below is the kernel.
#include "bc7_chain.h"
#include "bc7_dual.h"
#include "mfma_i8.h"
#include "bc7_bounds.h"

// HARD = false: the encoder.  A block whose mode-7 stage starts with at least A.hardMin partitions alive hands them to
// the second launch (A.hardCap slots; none left: it searches them itself) and records its best without them.
// HARD = true: the second launch.  kHardWaves (16) wavefronts per recorded block; each reloads the block's original wave
// (the group-wide booleans need its neighbours), searches one slice of the 64 mode-7 partitions against the recorded
// best and leaves its best candidate, packed, in A.hardCand; cvttmi_bc7_hard_commit_kernel picks the winner.
// Every candidate is compared by (error, position in the reference's order), so the split cannot change the result.
template <bool FAST, bool PT, bool HARD>
// (the body of the kernel as a function of its work item: the encoder's launches run it once per workgroup, the HARD launch
// loops a fixed-size grid over its items -- cvttmi_bc7_kernel below)
__device__ __forceinline__ void bc7Body(const uint8_t *__restrict__ blocks, uint8_t *__restrict__ out,
                                        const CvttBc7Args &A, const CvttDeviceTables *__restrict__ T,
                                        const CvttBc7DevicePlan *__restrict__ dplan, const u32 vBlock, const u32 vGrid)
{
    // error lower bound of every partition of the current mode, per block: the upper 16 bits of the binary32 value
    // (truncated, i.e. rounded down -- a bound may always be smaller).  Half the bytes of a float table: with that and 64
    // result slots the kernel fits 8 LDS granules = 16 workgroups per CU = 4 waves per SIMD.
    __shared__ unsigned short s_bound[64][16];
    // A bound is never negative, so its sign bit is free: it marks the entries that hold a second-tier (full-dimension)
    // bound already (lbStoreTier2), and readers take the absolute value (a source modifier, no instruction).
    auto lbLoadRaw = [&](int partition, int b) -> float { return __builtin_bit_cast(float, (u32)s_bound[partition][b] << 16); };
    auto lbLoad = [&](int partition, int b) -> float { return __builtin_fabsf(lbLoadRaw(partition, b)); };
    auto lbStore = [&](int partition, int b, float v) { s_bound[partition][b] = (unsigned short)(__builtin_bit_cast(u32, v) >> 16); };
    auto lbStoreTier2 = [&](int partition, int b, float v) { s_bound[partition][b] = (unsigned short)((__builtin_bit_cast(u32, v) >> 16) | 0x8000u); };
    // the same bytes as 32-bit words, [row][block], rows 1..16: where the dual-plane search parks its per-block invariants
    // (row 0 of the 16-bit table, the mode-6 bound, lies below them)
    u32 *const s_raw = reinterpret_cast<u32 *>(&s_bound[0][0]);
    __shared__ u32 s_pix[16][16];     // the 16 blocks of this wave
    __shared__ u32 s_blkFlags[16];    // wantPCA4 of the block's group
    __shared__ int s_scatter[16][14]; // raw sums (sum x per channel, sum x_r x_c) of every block: the scatter matrix of the bounds and the totals of the second tier come from here
    __shared__ u32 s_item[64];        // items of the current phase of a round: block | partition << 8 (up to 64 probes)
    __shared__ uint8_t s_myItems[PT ? 16 : 1][32]; // punch-through stages only: the items a block offered this round (elsewhere a block's items are consecutive)
    __shared__ UnitRec s_unit[64];    // PCA seeds per (item, subset)
    __shared__ u32 s_parked[16][2];   // the secondary index set of every block's best mode 4 / 5 candidate, out of the registers until the block is packed
    // the pixel bitmaps of the partitions (subset 1 of a two-subset partition; subsets 1 | 2 << 16 of a three-subset one): the
    // search looks them up per lane many times per round, and a per-lane lookup in the HBM tables is a dependent global load
    __shared__ float s_static[16];    // static alpha error of the RGB modes, whole block (BC67.cpp:1250-1264), times 0.9999
    __shared__ unsigned short s_pm2[64];
    __shared__ u32 s_pm3[64];
    // best of every (item, subset) = unit of the round: error, endpoints, indexes.  (During the dual-plane search the same
    // bytes hold the channel-major copy of the blocks, read with 128-bit loads.)
    __shared__ __attribute__((aligned(16))) u32 s_res[64][5];
    // BC7_RespectPunchThrough: the error of every trial (chain x refine round) of every unit of the round
    // [unit][chain][round], 32 x 16 x numRefine floats (punch-through instantiation only; up to kMaxPTRefine rounds)
    __shared__ float s_trialErr[PT ? 32 * 16 * kMaxPTRefine : 1];
    // ... and with more rounds than that (the reference only clamps refineRoundsBC7 from below, BC67.cpp:1044-1045) the
    // table of this wave lives in HBM; it is written and read inside the wave, between barriers
    float *const trialHbm = (PT && A.ptTrial) ? A.ptTrial + (size_t)vBlock * (size_t)(32 * 16) * (size_t)(A.refineRounds < 1 ? 1 : A.refineRounds) : nullptr;
    const cvttmi_bc7_plan *__restrict__ plan = &dplan->plan;
    // (not const: REFRESH_LANE() below hands the optimiser the same values as "new" ones at the start of every section of the
    // single-plane search, so that the LDS addresses and masks it derives from them are computed where they are used instead
    // of being hoisted in front of the stage loop and kept -- i.e. spilled -- across the chain rounds)
    int lane = threadIdx.x;
    int c = lane & 3;
    int blk = lane >> 2;
// (the lane number comes from v_mbcnt -- a workgroup is one wave -- so that not even threadIdx.x has to stay alive)
#define REFRESH_LANE() do { lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); asm volatile("" : "+v"(lane)); c = lane & 3; blk = lane >> 2; } while (0)
    u32 hardIndex = 0, hardBlock = 0;
    u64 hardMine = 0;
    float hardErr = FLT_MAX;
    int hardSeq = -1;
    if (HARD)
    {
        hardIndex = vBlock / kHardWaves;
        const u32 count = *A.hardCount;
        if (hardIndex >= (count < A.hardCap ? count : A.hardCap))
            return;
        const CvttBc7HardRec rec = A.hardRec[hardIndex];
        hardBlock = rec.blockIndex;
        hardErr = rec.err;
        hardSeq = rec.seq;
        // this wavefront's share: every kHardWaves-th of the partitions that were alive when the block was handed over
        u64 m = ((u64)rec.aliveHi << 32) | rec.aliveLo;
        const int q = (int)(vBlock % kHardWaves);
        for (int r = 0; m != 0; r++)
        {
            const u64 low = m & (0ull - m);
            if ((r % kHardWaves) == q)
                hardMine |= low;
            m ^= low;
        }
        if (hardMine == 0)
        {
            if (lane == 0)
                A.hardCand[vBlock].err = FLT_MAX;
            return;
        }
    }
    const u32 blockIndex = (HARD ? (hardBlock & ~15u) : vBlock * 16u) + (u32)(lane >> 2);
    const bool inRange = blockIndex < A.numBlocks;
#ifdef CVTT_BC7_BOUND_DUMP
    auto bdEmit = [&](u32 tier, u32 kind, u32 set, u32 mode, u32 numSub, u32 bits, u32 part, u32 sub, float computed, float stored, float err,
                      bool dropped, float x0 = 0.0f, float x1 = 0.0f, float x2 = 0.0f, float x3 = 0.0f) {
        boundDumpEmit(blockIndex, tier | (kind << 8) | (HARD ? 1u << 16 : 0u), set | (mode << 8) | (numSub << 16) | (bits << 24), part | (sub << 8),
                      computed, stored, err, dropped ? 1u : 0u, x0, x1, x2, x3);
    };
#endif
    // The per-lane predicates of the search live as bits of one register (`lf`) rather than as one lane mask each: the
    // scalar registers a mask takes (two each, for the whole kernel) are what the register allocator runs out of first.
    enum : u32 { LF_VALID = 1u, LF_ANY_ALPHA = 2u, LF_ALLOW_RGB = 4u, LF_ALLOW_M7 = 8u, LF_NONMAX_ALPHA = 16u };
    // HARD: the neighbours are loaded for the group-wide booleans only
    u32 lf = (inRange && (!HARD || blockIndex == hardBlock)) ? LF_VALID : 0u;
#define valid ((lf & LF_VALID) != 0)
#define anyBlockHasAlpha ((lf & LF_ANY_ALPHA) != 0)
#define allowRGBModes ((lf & LF_ALLOW_RGB) != 0)
#define allowMode7 ((lf & LF_ALLOW_M7) != 0)
#define blockHasNonMaxAlpha ((lf & LF_NONMAX_ALPHA) != 0)

    PROF_DECL
    s_pm2[lane] = T->partition2[lane];
    s_pm3[lane] = (u32)T->subsetMask3[lane][0] | ((u32)T->subsetMask3[lane][1] << 16);
    __syncthreads();
    u32 pix[16];
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(blocks + (size_t)(inRange ? blockIndex : 0u) * 64u);
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const uint4 v = src[i];
            pix[4 * i + 0] = v.x;
            pix[4 * i + 1] = v.y;
            pix[4 * i + 2] = v.z;
            pix[4 * i + 3] = v.w;
        }
        if (c == 0)
        {
#pragma unroll
            for (int i = 0; i < 4; i++)
                *reinterpret_cast<uint4 *>(&s_pix[lane >> 2][4 * i]) = make_uint4(pix[4 * i], pix[4 * i + 1], pix[4 * i + 2], pix[4 * i + 3]);
        }
    }

    REFRESH_LANE();
    // ---- per-block alpha statistics and the two group-wide booleans (BC67.cpp:1054-1078) ----
    int minAlpha = 255;
#pragma unroll
    for (int px = 0; px < 16; px++)
    {
        const int a = byteI(pix[px], 3);
        minAlpha = a < minAlpha ? a : minAlpha;
    }
    lf |= (minAlpha < 255) ? LF_NONMAX_ALPHA : 0u;
    const u64 ballotA = __ballot(minAlpha < 255);
    const u64 ballotR = __ballot(250 < minAlpha);
    const u32 groupA = (lane < 32) ? (u32)ballotA : (u32)(ballotA >> 32);
    const u32 groupR = (lane < 32) ? (u32)ballotR : (u32)(ballotR >> 32);
    lf |= (groupA != 0) ? LF_ANY_ALPHA : 0u;
    lf |= (groupR != 0) ? LF_ALLOW_RGB : 0u;
    const u64 mode7RGB = plan->mode7RGBPartitionEnabled;
    lf |= (groupA != 0 || mode7RGB != 0) ? LF_ALLOW_M7 : 0u;
    // RGBA seeds: PCA over 4 channels when the group has alpha or no RGB modes, otherwise the
    // RGB seeds extended with alpha = 255 (reference BC67.cpp:1113-1144)
    const bool wantPCA4 = anyBlockHasAlpha || !allowRGBModes;
    if (c == 0)
    {
        u32 f = wantPCA4 ? 1u : 0u;
        if (PT)
        {
            // BC67.cpp:1054-1067: punch-through = every alpha is 0 or 255
            bool isPunchThrough = true;
            int maxAlpha = 0;
#pragma unroll
            for (int px = 0; px < 16; px++)
            {
                const int a = byteI(pix[px], 3);
                isPunchThrough = isPunchThrough && (a == 0 || a == 255);
                maxAlpha = a > maxAlpha ? a : maxAlpha;
            }
            f |= (isPunchThrough ? 2u : 0u) | (maxAlpha > 0 ? 4u : 0u) | (blockHasNonMaxAlpha ? 8u : 0u);
        }
        s_blkFlags[lane >> 2] = f;
    }

    int numRefine = A.refineRounds;
    if (numRefine < 1)
        numRefine = 1;

    // Running best.  The reference walks candidates in a fixed order (single-plane modes
    // 0,1,2,3,6,7 by partition, then mode 4 / mode 5 by rotation and index selector) and
    // commits on a strict '<', i.e. it keeps the FIRST candidate that reaches the minimum.
    // We evaluate in a different order, so every candidate carries its position `seq` in the
    // reference's order and the commit compares (error, seq) lexicographically.
    // What is carried through the search is small: the error, `seq` -- which also names the mode, the partition or index
    // selector and the rotation (decoded when the block is packed) -- and the payload of the best candidate (three endpoint
    // pairs, 64 index bits), of which every lane of the quad keeps a quarter: sub-lane s < 3 the endpoints of subset s,
    // sub-lane 3 the indexes.  All four lanes take the same commit decisions, so the quarters always belong together.
    struct { float err; } work;
    work.err = HARD ? hardErr : FLT_MAX;
    int workSeq = HARD ? hardSeq : -1; // nothing committed yet: a candidate must beat FLT_MAX strictly
    u32 workPay0 = 0, workPay1 = 0;

    REFRESH_LANE();
    // ------------- whole-block scatter matrix: bounds for mode 6 and the four rotations -------------
    const bool prune = !HARD && A.prune != 0; // HARD: the bounds have been applied by the first launch
    BlockScatter bs;
    float lbRotMine = 0.0f; // sub-lane r: the bound of rotation r
    auto lbRotOf = [&](int rotation) -> float { return __shfl(lbRotMine, (lane & ~3) | rotation); };
    int rotOrder[4] = {0, 1, 2, 3};
    if (prune)
    {
        {
            int rs[4], rp[10];
            blockRawSumsQuad(pix, c, rs, rp);
            if (c == 0)
            {
#pragma unroll
                for (int i = 0; i < 10; i++)
                    s_scatter[lane >> 2][i] = rp[i];
#pragma unroll
                for (int i = 0; i < 4; i++)
                    s_scatter[lane >> 2][10 + i] = rs[i];
            }
            scatterFromRaw(rs, rp, A, bs);
        }
        if (!HARD)
        {
            Moments<4> m;
#pragma unroll
            for (int i = 0; i < 10; i++)
                m.cov[i] = bs.S[i];
            const float lbMode6 = shapeErrorLowerBound<4>(m, 16.0f, A.delta4);
            // mode 6 is the first single-plane stage: its bound waits where that stage looks for it
            if (c == 0)
                lbStore(0, lane >> 2, lbMode6);
            BOUND_DUMP(if (c == 0 && valid) bdEmit(BD_WHOLE6, BD_FORM, 3, 6, 1, 4, 0, 0, lbMode6, lbLoad(0, lane >> 2), work.err, false));
        }
        // rotation r codes channel r-1 (alpha for r = 0) on its own; the other three share a line
        if (!HARD)
        {
            const float s012 = A.wSqSum3;
            const float d0 = A.delta3;
            const float d1 = 0.5000005f * __builtin_amdgcn_sqrtf(s012 - A.wSq[0] + A.wSq[3]) * 1.000001f;
            const float d2 = 0.5000005f * __builtin_amdgcn_sqrtf(s012 - A.wSq[1] + A.wSq[3]) * 1.000001f;
            const float d3 = 0.5000005f * __builtin_amdgcn_sqrtf(s012 - A.wSq[2] + A.wSq[3]) * 1.000001f;
            // sub-lane r bounds rotation r (its three channels picked by selects, so that the quad runs the bound once)
            Moments<3> m;
#define pick(i0, i1, i2, i3) (c == 0 ? bs.S[i0] : c == 1 ? bs.S[i1] : c == 2 ? bs.S[i2] : bs.S[i3]) /* literal indexes: bs.S stays in registers */
            // channel triples (a < b < c'): rotation 0: 0 1 2, 1: 1 2 3, 2: 0 2 3, 3: 0 1 3
            m.cov[0] = pick(tri(0, 0), tri(1, 1), tri(0, 0), tri(0, 0)); // (a, a)
            m.cov[1] = pick(tri(1, 0), tri(2, 1), tri(2, 0), tri(1, 0)); // (b, a)
            m.cov[2] = pick(tri(1, 1), tri(2, 2), tri(2, 2), tri(1, 1)); // (b, b)
            m.cov[3] = pick(tri(2, 0), tri(3, 1), tri(3, 0), tri(3, 0)); // (c', a)
            m.cov[4] = pick(tri(2, 1), tri(3, 2), tri(3, 2), tri(3, 1)); // (c', b)
            m.cov[5] = pick(tri(2, 2), tri(3, 3), tri(3, 3), tri(3, 3)); // (c', c')
#undef pick
            lbRotMine = shapeErrorLowerBound<3>(m, 16.0f, c == 0 ? d0 : c == 1 ? d1 : c == 2 ? d2 : d3);
            BOUND_DUMP(if (valid) bdEmit(BD_ROT, BD_FORM, 3, 4, 1, 4, (u32)c, 0, lbRotMine, lbRotMine, work.err, false, c == 0 ? d0 : c == 1 ? d1 : c == 2 ? d2 : d3));
        }
        // search the rotations in the order of their bounds summed over the wave: the likely
        // winner first, so that the others meet a tight best error
        float tot[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < 4 && !HARD; r++)
        {
            float t = valid ? lbRotOf(r) : 0.0f;
#pragma unroll
            for (int step = 1; step < 64; step <<= 1)
                t += xorLane(t, step);
            tot[r] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t)));
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
        {
            int rank = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (q != r && (tot[q] < tot[r] || (tot[q] == tot[r] && q < r)))
                    rank++;
#pragma unroll
            for (int slot = 0; slot < 4; slot++)
                if (rank == slot)
                    rotOrder[slot] = r;
        }
    }
    PROF_MARK(6)

    // ================================ dual-plane modes 4,5 ================================
    // reference TryDualPlane, BC67.cpp:1678-1963.  The RGB seeds depend only on the rotation,
    // so sub-lane r computes them for rotation r once (the reference recomputes them for each
    // mode / index selector).
    REFRESH_LANE();
    if constexpr (!HARD)
    {
        Unfinished uRot;
        {
            u32 rpix[16];
#pragma unroll
            for (int px = 0; px < 16; px++)
                rpix[px] = rotatePixel(pix[px], c);
            float lw[4];
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
                lw[ch] = A.w[ch];
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
                if (c == ch + 1)
                {
                    lw[ch] = A.w[3];
                    lw[3] = A.w[ch];
                }
            pcaEndpoints<3>(rpix, 0xffffu, lw, -1, uRot);
        }
        // the seeds of rotation r wait in s_unit[quad | r] (idle until the single-plane stages): a step reads the ones of its
        // rotation from there instead of every lane keeping its own through all twelve steps
#pragma unroll
        for (int ch = 0; ch < 4; ch++)
        {
            s_unit[lane].base[ch] = uRot.base[ch];
            s_unit[lane].offset[ch] = uRot.offset[ch];
        }
        PROF_MARK(0)

        // fast indexing: the search reads a channel-major copy of the block -- per group g of four pixels one word per channel
        // position, in the channel order of the rotation being searched -- from s_P (= s_res, idle until the single-plane
        // stages; 20 words per block so that the 128-bit loads of a wave spread over the banks).  Sub-lane g builds group g
        // from the pixel-major copy whenever the rotation changes (at most four times per wave).
        u32 *const s_P = &s_res[0][0] + (lane >> 2) * 20;
        auto writeRotated = [&](int rotation) {
            const uint4 q = *reinterpret_cast<const uint4 *>(&s_pix[lane >> 2][4 * c]);
            const u32 ab02 = __builtin_amdgcn_perm(q.y, q.x, 0x06020400u); // a0 b0 a2 b2
            const u32 ab13 = __builtin_amdgcn_perm(q.y, q.x, 0x07030501u); // a1 b1 a3 b3
            const u32 cd02 = __builtin_amdgcn_perm(q.w, q.z, 0x06020400u);
            const u32 cd13 = __builtin_amdgcn_perm(q.w, q.z, 0x07030501u);
            u32 w0 = __builtin_amdgcn_perm(cd02, ab02, 0x05040100u); // a0 b0 c0 d0
            u32 w2 = __builtin_amdgcn_perm(cd02, ab02, 0x07060302u); // a2 b2 c2 d2
            u32 w1 = __builtin_amdgcn_perm(cd13, ab13, 0x05040100u);
            u32 w3 = __builtin_amdgcn_perm(cd13, ab13, 0x07060302u);
            // rotation r > 0 exchanges channel r - 1 with alpha (reference BC67.cpp:1695-1698)
            if (rotation == 1) { const u32 t = w0; w0 = w3; w3 = t; }
            if (rotation == 2) { const u32 t = w1; w1 = w3; w3 = t; }
            if (rotation == 3) { const u32 t = w2; w2 = w3; w3 = t; }
            *reinterpret_cast<uint4 *>(s_P + 4 * c) = make_uint4(w0, w1, w2, w3);
        };
        // what every configuration of a rotation would otherwise recompute (DualInv), per original channel: sub-lane ch
        // takes channel ch and parks the five values in rows 1..16 of s_raw (= s_bound), which is idle until the partition bounds
        // (row 0 of the 16-bit table holds the mode-6 bound); a step reads the rows its rotation needs
        {
            __syncthreads(); // s_pix is complete
            writeRotated(0);
            __syncthreads();
            u32 mine[4];
#pragma unroll
            for (int g = 0; g < 4; g++)
                mine[g] = s_P[4 * g + c];
            const float wc = (c == 0) ? A.w[0] : (c == 1) ? A.w[1] : (c == 2) ? A.w[2] : A.w[3];
            u32 sq = 0, su = 0;
            int mn = 255, mx = 0;
            float sw = 0.0f; // sum of x * w in pixel order: the refiner's m_v
#pragma unroll
            for (int g = 0; g < 4; g++)
            {
                sq = __builtin_amdgcn_udot4(mine[g], mine[g], sq, false);
                su = __builtin_amdgcn_udot4(mine[g], 0x01010101u, su, false);
#pragma unroll
                for (int k = 0; k < 4; k++)
                {
                    const int a = byteI(mine[g], k);
                    mn = a < mn ? a : mn;
                    mx = a > mx ? a : mx;
                    sw = sw + byteF(mine[g], k) * wc;
                }
            }
            s_raw[(1 + c) * 16 + (lane >> 2)] = sq;
            s_raw[(5 + c) * 16 + (lane >> 2)] = (u32)mn | ((u32)mx << 8);
            s_raw[(9 + c) * 16 + (lane >> 2)] = __builtin_bit_cast(u32, sw);
            s_raw[(13 + c) * 16 + (lane >> 2)] = __builtin_bit_cast(u32, (float)(int)su); // exact
        }
        __syncthreads();
        // slow indexing reads the pixels pixel-major, rotated, from the same LDS bytes (written before its first step)
        auto writeRotatedPixels = [&](int rotation) {
            const uint4 q = *reinterpret_cast<const uint4 *>(&s_pix[lane >> 2][4 * c]);
            *reinterpret_cast<uint4 *>(s_P + 4 * c) = make_uint4(rotatePixel(q.x, rotation), rotatePixel(q.y, rotation),
                                                                 rotatePixel(q.z, rotation), rotatePixel(q.w, rotation));
        };
        int curRotation = FAST ? 0 : -1;
#ifdef CVTT_BC7_PROFILE
        float simKey[12], simErr[12];
        int simN = 0;
#endif
        for (int step = 0; step < 12; step++)
        {
            REFRESH_LANE();
            const int slot = step / 3, which = step - slot * 3;
            const int rotation = (slot == 0) ? rotOrder[0] : (slot == 1) ? rotOrder[1] : (slot == 2) ? rotOrder[2] : rotOrder[3];
            // position in the reference's commit order: mode 4 (rot 0: is 0,1; rot 1: ...), then mode 5 rot 0..3
            const int mode = which < 2 ? 4 : 5;
            const int indexSelector = which < 2 ? which : 0;
            const int cfg = which < 2 ? rotation * 2 + which : 8 + rotation;
            int numTweak = (mode == 4) ? plan->mode4SP[rotation][indexSelector] : plan->mode5SP[rotation];
            if (numTweak <= 0)
                continue;
            if (numTweak > 4)
                numTweak = 4;
            if (prune)
            {
                // the second plane costs >= 0, the first at least the bound of its three channels
                const float lb = lbRotOf(rotation);
                // (word 8: 1 = the whole wave skipped the step; a block whose bound exceeds its best is searched along with the others otherwise)
                BOUND_DUMP(if (valid && c == 0) bdEmit(BD_ROT, BD_RELOAD, 3, (u32)mode, 1, (u32)indexSelector, (u32)rotation, 0, lb, lb, work.err, lb > work.err,
                                                       __ballot(valid && !(lb > work.err)) == 0 ? 1.0f : 0.0f));
                if (__ballot(valid && !(lb > work.err)) == 0)
                    continue;
            }

            if (rotation != curRotation)
            {
                if (FAST)
                {
                    __syncthreads(); // everybody is done with the previous rotation's copy
                    writeRotated(rotation);
                    __syncthreads();
                }
                else
                {
                    __syncthreads();
                    writeRotatedPixels(rotation);
                    __syncthreads();
                }
                curRotation = rotation;
            }
            float rw[4], rwSq[4], rrcpW[4];
#pragma unroll
            for (int ch = 0; ch < 4; ch++)
            {
                rw[ch] = A.w[ch];
                rwSq[ch] = A.wSq[ch];
                rrcpW[ch] = A.rcpW[ch];
            }
#pragma unroll
            for (int ch = 0; ch < 3; ch++)
                if (rotation == ch + 1)
                {
                    rw[ch] = A.w[3];
                    rwSq[ch] = A.wSq[3];
                    rrcpW[ch] = A.rcpW[3];
                    rw[3] = A.w[ch];
                    rwSq[3] = A.wSq[ch];
                    rrcpW[3] = A.rcpW[ch];
                }

            PROF_COUNT(0, 16)
            PROF_COUNT(1, __popcll(__ballot(valid && c == 0 && !(lbRotOf(rotation) > work.err))))
            Unfinished u;
            {
                const UnitRec &ur = s_unit[(lane & ~3) | rotation];
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                {
                    u.base[ch] = ur.base[ch];
                    u.offset[ch] = ur.offset[ch];
                }
            }
            ShapeBest b, bA;
            {
                DualInv inv;
                const int sepCh = (rotation == 0) ? 3 : rotation - 1; // the original channel that is coded on its own
                inv.words = s_raw + (lane >> 2);
#pragma unroll
                for (int ch = 0; ch < 3; ch++)
                {
                    const int orig = (rotation == ch + 1) ? 3 : ch;
                    inv.rowSq[ch] = (1 + orig) * 16;
                    inv.rowVs[ch] = (9 + orig) * 16;
                }
                inv.rowSq[3] = (1 + sepCh) * 16;
                inv.rowVs[3] = (13 + sepCh) * 16;
                inv.minMax = s_raw[(5 + sepCh) * 16 + (lane >> 2)];
                evalDual<FAST>(s_P, inv, mode, indexSelector, u, numTweak, rw, rwSq, rrcpW, A.flags, T, numRefine, lane, b, bA);
            }

            const float combined = b.err + bA.err; // reference BC67.cpp:1942
            const int seq = 384 + cfg;
#ifdef CVTT_BC7_PROFILE
            {
                const float lbp = lbRotOf(rotation);
                const bool needed = valid && c == 0 && !(lbp > work.err);
                PROF_COUNT(6, (needed && (bA.err + lbp > work.err)) ? 1 : 0)
                if (needed && simN < 12)
                {
                    simKey[simN] = lbp + bA.err;
                    simErr[simN] = combined;
                    simN++;
                }
            }
#endif
            if (combined < work.err || (combined == work.err && seq < workSeq))
            {
                work.err = combined;
                workSeq = seq;
                // index selector 1: the 2-bit set is the alpha plane (BC67.cpp:1953-1957)
                const u32 iLo = indexSelector ? bA.idxLo : b.idxLo, iHi = indexSelector ? bA.idxHi : b.idxHi;
                workPay0 = (c == 0) ? (b.ep0 | bA.ep0) : (c == 3) ? iLo : 0u;
                workPay1 = (c == 0) ? (b.ep1 | bA.ep1) : (c == 3) ? iHi : 0u;
                s_parked[lane >> 2][0] = indexSelector ? b.idxLo : bA.idxLo;
                s_parked[lane >> 2][1] = indexSelector ? b.idxHi : bA.idxHi;
            }
        }
#ifdef CVTT_BC7_PROFILE
        {
            // how many colour planes an alpha-plane-first, best-key-first order would have to evaluate
            float best = FLT_MAX;
            int evald = 0;
            u32 left = (1u << simN) - 1u;
            while (left)
            {
                int pick = -1;
                float pk = FLT_MAX;
                for (int i = 0; i < 12; i++)
                    if (((left >> i) & 1u) && (pick < 0 || simKey[i] < pk))
                    {
                        pick = i;
                        pk = simKey[i];
                    }
                if (pk > best)
                    break;
                evald++;
                best = simErr[pick] < best ? simErr[pick] : best;
                left &= ~(1u << pick);
            }
            PROF_COUNT(7, evald)
        }
#endif
        __syncthreads();
        PROF_MARK(1)
    }

    // =========================== single-plane modes 0,1,2,3,6,7 ===========================
    // reference TrySinglePlane, BC67.cpp:1146-1660.  Per mode: the partitions that can still
    // win (bounds in LDS vs the best error so far) form a wave-uniform survivor list, which is
    // consumed in batches of four (partition, subset) items: sub-lane c runs the PCA seed search
    // of item c (per-lane shape mask), then the items are searched one after the other with the
    // shape wave-uniform.
    // pixel bitmap of subset `sub` of partition `partition` of a mode with numSub subsets
    auto subsetMaskOf = [&](int numSub, int partition, int sub) -> u32 {
        if (numSub == 1)
            return 0xffffu;
        if (numSub == 2)
        {
            const u32 m1 = s_pm2[partition];
            return sub ? m1 : (~m1 & 0xffffu);
        }
        const u32 m = s_pm3[partition];
        const u32 m1 = m & 0xffffu, m2 = m >> 16;
        return sub == 1 ? m1 : sub == 2 ? m2 : (~(m1 | m2) & 0xffffu);
    };
    // From here on the pixel-major block is read from LDS where it is needed (the bounds): 16 registers that the chain
    // rounds, which have the fewest to spare, do not have to carry.
    auto pixFromLds = [&](u32 (&px)[16]) {
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const uint4 v = *reinterpret_cast<const uint4 *>(&s_pix[blk][4 * i]);
            px[4 * i + 0] = v.x;
            px[4 * i + 1] = v.y;
            px[4 * i + 2] = v.z;
            px[4 * i + 3] = v.w;
        }
    };
    // Wave-uniform bookkeeping of the bounds, packed into one word of 3-bit fields (six separate ints were six VGPRs to the
    // register allocator, which cannot tell that they are uniform: they were the first to be spilled):
    //   WS_BOUNDS_FOR  which bound set s_bound holds, plus one: 1 = two subsets RGBA, 2 = two subsets RGB, 3 = three subsets RGB,
    //                  4 = mode 6; 0 = none.  (Which of its entries have had the second-tier bound merged in is marked in the
    //                  entries themselves: lbStoreTier2.)
    //   WS_T2_NOPAY    the second tier removed nothing in a stage with this many index bits: not again, unless a mode has fewer
    //   WS_SHARP_NOPAY the same for its second, sharper pass;  WS_STRIKES: and for the sharper bound in the filter of the probes
    //   WS_BOUND_BITS  The second-tier bounds know how many index levels the mode has, and a set of bounds is shared by modes with
    //                  three and with two index bits: what is in the table holds for modes with at most this many index bits
    //                  (4 = first tier only, any mode).  The stage orders run the three-bit mode of a set first; its bounds are
    //                  valid for the two-bit mode that follows, which computes its own, sharper ones for what is still alive then.
    //   WS_SHARP_RAN   The marks in the table say "has the plain second-tier bound" (which knows no levels); that the sharper
    //                  pass has been over the set for a number of index bits is remembered here (the partitions alive in a later
    //                  stage of the same set were alive then, too).
    enum : int { WS_BOUNDS_FOR = 0, WS_BOUND_BITS = 3, WS_SHARP_RAN = 6, WS_SHARP_NOPAY = 9, WS_T2_NOPAY = 12, WS_STRIKES = 15 };
    u32 ws = (4u << WS_BOUND_BITS) | (4u << WS_SHARP_RAN);
#define WS_GET(f) ((int)((ws >> (f)) & 7u))
#define WS_SET(f, v) do { ws = (u32)__builtin_amdgcn_readfirstlane((int)((ws & ~(7u << (f))) | ((u32)(v) << (f)))); } while (0)
    // static alpha error of the RGB modes, whole block (BC67.cpp:1250-1264)
    // (kept in LDS, one float per block: in a register it lives through every chain round for the sake of two additions per
    // stage -- and gets spilled)
    if (c == 0)
        s_static[blk] = 0.0f;
    if (prune)
    {
        u32 acc = 0;
        u32 lpix[16];
        pixFromLds(lpix);
#pragma unroll
        for (int px = 0; px < 16; px++)
        {
            const int d = 255 - byteI(lpix[px], 3);
            acc = (u32)mad24(d, d, (int)acc);
        }
        if (c == 0)
            s_static[blk] = ((A.flags & CVTTMI_FLAG_UNIFORM) ? (float)(int)acc : (float)(int)acc * A.wSq[3]) * 0.9999f;
    }

    for (int stageOrder = 0; stageOrder < 6; stageOrder++)
    {
        // The order of the stages is free (every commit compares (error, position in the reference's order)).  A wave without a
        // single translucent pixel searches modes 1 and 3 before mode 7: there mode 7 -- the same partitions with coarser end
        // points -- almost never wins, and what the other two find first prunes its partitions (smooth opaque gradients: 44
        // -> ... partitions per block alive in mode 7); the three share one set of bounds.
        REFRESH_LANE();
        const int stageIter = (ballotA == 0 && !HARD) ? ((stageOrder == 1) ? 2 : (stageOrder == 2) ? 3 : (stageOrder == 3) ? 1 : stageOrder) : stageOrder;
        ModeDesc md;
        int numSubsets, numPartitions, stage, boundSet;
        switch (stageIter)
        {
        case 0: stage = 4; md = {6, 4, 4, 7, 0}; numSubsets = 1; numPartitions = 1; boundSet = 3; break;
        case 1: stage = 5; md = {7, 2, 4, 5, 6}; numSubsets = 2; numPartitions = 64; boundSet = 0; break;
        case 2: stage = 1; md = {1, 3, 2, 6, 7}; numSubsets = 2; numPartitions = 64; boundSet = 1; break;
        case 3: stage = 3; md = {3, 2, 4, 7, 0}; numSubsets = 2; numPartitions = 64; boundSet = 1; break;
        case 4: stage = 0; md = {0, 3, 4, 4, 5}; numSubsets = 3; numPartitions = 16; boundSet = 2; break;
        default: stage = 2; md = {2, 2, 1, 5, 5}; numSubsets = 3; numPartitions = 64; boundSet = 2; break;
        }
        if (HARD && stageIter != 1)
            continue; // the second launch searches mode-7 partitions only
        // A wave without a single translucent pixel: the RGBA bounds of mode 7 would equal the RGB bounds of modes 1 / 3
        // (no variance in alpha; the colour part of a trial's error is bounded by the three-channel bound whatever alpha
        // does), so mode 7 takes the RGB set and the next stage finds its bounds already there.
        if (stageIter == 1 && ballotA == 0)
            boundSet = 1;
        const int mode = md.mode;
        const bool isRGB = mode < 4;
        // does this mode run for my group?  (wave-uniform skip when it runs for nobody -- before the plan is read: a
        // scalar load from memory per stage that a wave of alpha blocks would wait on four times for nothing)
        const bool laneRuns = isRGB ? allowRGBModes : (mode == 7 ? allowMode7 : true);
        if (__ballot(laneRuns) == 0)
            continue;
        u64 enabled;
        switch (stageIter)
        {
        case 0: enabled = plan->mode6Enabled ? 1 : 0; break;
        case 1: enabled = ~0ull; break; // dead mask in the reference (BC67.cpp:1592-1597)
        case 2: enabled = plan->mode1PartitionEnabled; break;
        case 3: enabled = plan->mode3PartitionEnabled; break;
        case 4: enabled = plan->mode0PartitionEnabled & 0xffffull; break;
        default: enabled = plan->mode2PartitionEnabled; break;
        }
        if (HARD)
            enabled = hardMine; // this wavefront's slice of the mode-7 partitions
        if (enabled == 0)
            continue;

        // ---- bounds of every partition of this mode (shared by the modes with the same subsets/channels) ----
        u32 freshAlive = 0;      // bit k: the bound of partition 4k + c, computed just now, does not exceed the block's best error
        bool freshBounds = false;
        if (prune)
        {
            if (WS_GET(WS_BOUNDS_FOR) == boundSet + 1 && WS_GET(WS_BOUND_BITS) < md.indexBits)
                WS_SET(WS_BOUNDS_FOR, 0); // (no stage order does this: two-bit bounds in the table and a three-bit mode to search)
            if (WS_GET(WS_BOUNDS_FOR) != boundSet + 1)
            {
                WS_SET(WS_BOUND_BITS, 4);
                WS_SET(WS_SHARP_RAN, 4);
                __syncthreads();
                if (boundSet == 3)
                {
                    // written when the block statistics were computed
                }
                else
                {
                    const bool use4 = (boundSet == 0);
                    auto boundsOnGrid = [&](auto g8) {
                    constexpr bool G8 = decltype(g8)::value;
                    const float wsum = A.wSqSum3 + (use4 ? A.wSq[3] : 0.0f);
                    const float scale = (G8 ? kBoundGrid8 : kBoundGrid16) / (255.0f * __builtin_amdgcn_sqrtf(wsum)); // wave-uniform
                    const float invScaleSq = 1.0f / (scale * scale);
                    // rounding the projected points moves each by at most sqrt(2)/2 grid units
                    const float twoDelta = 2.0f * ((use4 ? A.delta4 : A.delta3) + 0.7072f / scale);
                    // formed once per bound set, not per partition (machine LICM is off for this file): the static alpha error
                    // of the RGB sets, and 1/n of every subset size, lane n of one register (read with ds_bpermute: the
                    // crossbar, no LDS bytes; every lane is active here, and a lane that were not would read 0 = a smaller bound)
                    const float staticErr = use4 ? 0.0f : s_static[blk];
                    const int rcpLane = (int)kRcpDown[lane < 16 ? lane : 16];
                    auto rcpOf = [&](int n) -> float { return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(n << 2, rcpLane)); };
                    Proj2D<G8> P;
                    PROF_MARK(2)
                    {
                        // take the block statistics back from LDS (they were not kept in registers across the search)
                        BlockScatter bsL;
                        {
                            int rs[4], rp[10];
#pragma unroll
                            for (int i = 0; i < 10; i++)
                                rp[i] = s_scatter[blk][i];
#pragma unroll
                            for (int i = 0; i < 4; i++)
                                rs[i] = s_scatter[blk][10 + i];
                            scatterFromRaw(rs, rp, A, bsL);
                        }
                        u32 lpix[16];
                        pixFromLds(lpix);
                        makeProjection(lpix, bsL, A, use4, scale, P);
                    }
                    PROF_MARK(7)
                    bool byMatrix = false;
                    if constexpr (G8)
                        byMatrix = boundSet < 2;
                    if constexpr (G8)
                    if (byMatrix)
                    {
                        // Two subsets on the 8-bit grid: the masked sums come from the matrix cores (bc7_bounds.h, "by the
                        // matrix cores").  The records of the blocks and the alive words behind them lie in s_res, idle between
                        // the rounds of one stage and the next.  Lane l of a result is partition 32 tile + (l & 31) of the
                        // blocks 4 g + 2 j + (l >> 5), j = 0, 1: sixteen bounds per lane, as in the loop below.
                        u32 *const s_t1 = &s_res[0][0];
                        if (c == 0)
                        {
                            uint4 *const rec = reinterpret_cast<uint4 *>(s_t1 + blk * kT1RecWords);
                            rec[0] = make_uint4(P.U[0], P.U[1], P.U[2], P.U[3]);
                            rec[1] = make_uint4(P.V[0], P.V[1], P.V[2], P.V[3]);
                            rec[2] = make_uint4((u32)P.tU, (u32)P.tV, (u32)P.tUU, (u32)P.tVV);
                            rec[3] = make_uint4((u32)P.tUV, __builtin_bit_cast(u32, work.err), __builtin_bit_cast(u32, staticErr), 0u);
                        }
                        __syncthreads();
                        const int h = lane >> 5;
                        u64 maskOp[2];
                        int n1[2];
                        float rcp1[2], rcp0[2];
#pragma unroll
                        for (int t = 0; t < 2; t++)
                        {
                            const u32 m = s_pm2[(lane & 31) + 32 * t];
                            maskOp[t] = t1MaskOperand(m, h);
                            n1[t] = __popc(m);
                            rcp1[t] = __builtin_bit_cast(float, kRcpDown[n1[t]]);
                            rcp0[t] = __builtin_bit_cast(float, kRcpDown[16 - n1[t]]);
                        }
                        const int rowQ = t1RowQuantity(lane & 31);
                        const u32 *const featRec = s_t1 + t1RowBlock(lane & 31) * kT1RecWords;
#pragma unroll 1
                        for (int g = 0; g < 4; g++)
                        {
                            const u64 featOp = t1FeatureOperand(featRec + 4 * g * kT1RecWords, h, rowQ);
#pragma unroll
                            for (int t = 0; t < 2; t++)
                            {
                                const v16i zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                                const v16i acc = mfmaI8(featOp, maskOp[t], zero);
                                const int partition = (lane & 31) + 32 * t;
#pragma unroll
                                for (int j = 0; j < 2; j++)
                                {
                                    const int block = 4 * g + 2 * j + h;
                                    const uint4 tot = *reinterpret_cast<const uint4 *>(s_t1 + block * kT1RecWords + 8);
                                    const uint4 tail = *reinterpret_cast<const uint4 *>(s_t1 + block * kT1RecWords + 12);
                                    Sums2D s1, s0;
                                    s1.n = n1[t];
                                    s1.u = acc[8 * j + 0];
                                    s1.v = acc[8 * j + 1];
                                    s1.uu = acc[8 * j + 2] + (int)((u32)acc[8 * j + 3] << 7);
                                    s1.vv = acc[8 * j + 4] + (int)((u32)acc[8 * j + 5] << 7);
                                    s1.uv = acc[8 * j + 6] + (int)((u32)acc[8 * j + 7] << 7);
                                    s0.n = 16 - s1.n;
                                    s0.u = (int)tot.x - s1.u;
                                    s0.v = (int)tot.y - s1.v;
                                    s0.uu = (int)tot.z - s1.uu;
                                    s0.vv = (int)tot.w - s1.vv;
                                    s0.uv = (int)tail.x - s1.uv;
                                    const float blockErr = __builtin_bit_cast(float, tail.y);
                                    float lb = subsetBound2D<true>(s0, rcp0[t], invScaleSq, twoDelta) + subsetBound2D<true>(s1, rcp1[t], invScaleSq, twoDelta);
                                    lb += __builtin_bit_cast(float, tail.z); // the static alpha error (lb >= +0: adding 0.0f changes nothing)
                                    lbStore(partition, block, lb);
                                    BOUND_DUMP(if (vBlock * 16u + (u32)block < A.numBlocks)
                                                   boundDumpEmit(vBlock * 16u + (u32)block, BD_TIER1 | (BD_FORM_CMP << 8), (u32)boundSet | ((u32)mode << 8) | ((u32)numSubsets << 16) | (4u << 24),
                                                                 (u32)partition, lb, lbLoad(partition, block), blockErr, lb > blockErr ? 1u : 0u,
                                                                 __builtin_bit_cast(float, tail.z), 0.0f, 0.0f, 0.0f));
                                    // the comparison on the full-precision value, as ballots per block
                                    const u64 stay = __ballot(!(lb > blockErr));
                                    if (lane == 0)
                                        *reinterpret_cast<uint2 *>(s_t1 + kT1AliveAt + 16 * t + 4 * g + 2 * j) = make_uint2((u32)stay, (u32)(stay >> 32));
                                }
                            }
                        }
                        __syncthreads();
                        freshAlive = everyFourth((u64)s_t1[kT1AliveAt + blk] | ((u64)s_t1[kT1AliveAt + 16 + blk] << 32), c);
                        freshBounds = true;
                        return;
                    }
                    // the byte masks of the next partition are loaded while this one is computed
                    const bool two = !G8 && boundSet < 2; // (on the 8-bit grid the two-subset sets went to the matrix cores above)
                    auto selOf = [&](int partition, int which) -> uint4 {
                        return *reinterpret_cast<const uint4 *>(T->subsetByteMask[two ? partition : 64 + 2 * partition + which]);
                    };
                    uint4 selA = make_uint4(0, 0, 0, 0), selB = make_uint4(0, 0, 0, 0);
                    if constexpr (G8)
                    {
                        selA = selOf(c, 0);
                        if (!two)
                            selB = selOf(c, 1);
                    }
                    for (int k = 0; k < 16; k++)
                    {
                        const int partition = 4 * k + c;
                        float lb;
                        uint4 selA1 = selA, selB1 = selB;
                        if constexpr (G8)
                        {
                            const int nextPartition = (k < 15 ? partition + 4 : partition);
                            selA1 = selOf(nextPartition, 0);
                            if (!two)
                                selB1 = selOf(nextPartition, 1);
                        }
                        if (two)
                        {
                            Sums2D s1, s0;
                            if constexpr (G8)
                                maskedSumsSel(P, __popc((u32)s_pm2[partition]), selA, s1);
                            else
                                maskedSums(P, s_pm2[partition], s1);
                            s0.n = 16 - s1.n;
                            s0.u = P.tU - s1.u;
                            s0.v = P.tV - s1.v;
                            s0.uu = P.tUU - s1.uu;
                            s0.vv = P.tVV - s1.vv;
                            s0.uv = P.tUV - s1.uv;
                            lb = subsetBound2D<G8>(s0, rcpOf(s0.n), invScaleSq, twoDelta) + subsetBound2D<G8>(s1, rcpOf(s1.n), invScaleSq, twoDelta);
                        }
                        else
                        {
                            Sums2D s1, s2, s0;
                            if constexpr (G8)
                            {
                                maskedSumsSel(P, __popc(s_pm3[partition] & 0xffffu), selA, s1);
                                maskedSumsSel(P, __popc(s_pm3[partition] >> 16), selB, s2);
                            }
                            else
                            {
                            maskedSums(P, s_pm3[partition] & 0xffffu, s1);
                            maskedSums(P, s_pm3[partition] >> 16, s2);
                            }
                            s0.n = 16 - s1.n - s2.n;
                            s0.u = P.tU - s1.u - s2.u;
                            s0.v = P.tV - s1.v - s2.v;
                            s0.uu = P.tUU - s1.uu - s2.uu;
                            s0.vv = P.tVV - s1.vv - s2.vv;
                            s0.uv = P.tUV - s1.uv - s2.uv;
                            lb = subsetBound2D<G8>(s0, rcpOf(s0.n), invScaleSq, twoDelta) + subsetBound2D<G8>(s1, rcpOf(s1.n), invScaleSq, twoDelta) +
                                 subsetBound2D<G8>(s2, rcpOf(s2.n), invScaleSq, twoDelta);
                        }
                        lb += staticErr; // (lb >= +0: adding 0.0f changes nothing)
                        lbStore(partition, blk, lb);
                        BOUND_DUMP(if (valid) bdEmit(BD_TIER1, BD_FORM_CMP, (u32)boundSet, (u32)mode, (u32)numSubsets, 4, (u32)partition, 0, lb, lbLoad(partition, blk),
                                                     work.err, lb > work.err, staticErr));
                        freshAlive |= (lb > work.err) ? 0u : (1u << k);
                        selA = selA1;
                        selB = selB1;
                    }
                    freshBounds = true;
                    };
                    if (use4 ? CVTT_GRID8_RGBA : CVTT_GRID8_RGB)
                        boundsOnGrid(std::true_type{});
                    else
                        boundsOnGrid(std::false_type{});
                }
                __syncthreads();
                WS_SET(WS_BOUNDS_FOR, boundSet + 1);
            }
        }
        PROF_MARK(2)

        // ---- every block offers its cheapest-bound candidate partition per round, until the bound
        // of the next one exceeds its best error.  Sub-lane c keeps the candidates 4k+c.
        // The offers of a round are searched by the whole wave: one lane per chain. ----
        const int CP = md.numP * 4;         // chains per subset: p-bit combinations x seed points
        const int UPB = 64 / CP;            // subsets searched at once
        // bit k: partition 4k + c is enabled for this block and its bound does not rule it out
        u32 aliveBits = (valid && laneRuns) ? everyFourth(enabled, c) : 0u; // `enabled` has no bits past the mode's partitions
        if (mode == 7 && anyBlockHasAlpha && !blockHasNonMaxAlpha)
            aliveBits &= everyFourth(mode7RGB, c); // BC67.cpp:1625-1635: this lane may not take the other partitions
        u32 tier2Done = 0; // bit k: partition 4k + c has its second-tier bound (none has when the bounds are fresh)
        if (prune)
        {
            if (freshBounds)
                aliveBits &= freshAlive; // compared while the bounds were computed: the best error has not moved since
            else
            {
                for (int k = 0; k * 4 < numPartitions; k++)
                {
                    const float raw = lbLoadRaw(4 * k + c, blk);
                    // (the tier of a marked entry: the sharper pass has been over the set iff WS_SHARP_RAN says so)
                    BOUND_DUMP(if ((aliveBits >> k) & 1u) bdEmit(boundSet == 3 ? BD_WHOLE6 : (__builtin_bit_cast(u32, raw) >> 31) ? (WS_GET(WS_SHARP_RAN) < 4 ? BD_SHARP : BD_FULL) : BD_TIER1,
                                                                 BD_RELOAD, (u32)boundSet, (u32)mode, (u32)numSubsets, (u32)md.indexBits, (u32)(4 * k + c), 0,
                                                                 __builtin_fabsf(raw), __builtin_fabsf(raw), work.err, __builtin_fabsf(raw) > work.err, (float)WS_GET(WS_BOUND_BITS)));
                    if (__builtin_fabsf(raw) > work.err)
                        aliveBits &= ~(1u << k);
                    tier2Done |= (__builtin_bit_cast(u32, raw) >> 31) << k;
                }
            }
        }

        if (prune && numSubsets >= 2)
        {
            // second tier: full-dimension bounds of the partitions that are still alive and have none yet.  A partition
            // costs about a fifth of a chain pass here and a seed pass plus chain passes if it stays.  Two passes: the plain
            // bound (subsetBoundFull) for all of them; then the sharper one (subsetBoundSharp, three times the work) for what the
            // first pass left -- on noise-like content that is little, and nothing of it goes, so a wave that sees the second
            // pass remove nothing does not run it again for modes with as many index bits.
            const bool sharpPays = WS_GET(WS_SHARP_NOPAY) == 0 || md.indexBits < WS_GET(WS_SHARP_NOPAY);
            const u32 todo = aliveBits & ~tier2Done;
            const bool tier2Pays = WS_GET(WS_T2_NOPAY) == 0 || md.indexBits < WS_GET(WS_T2_NOPAY);
            const bool runPlain = tier2Pays && __ballot(todo != 0) != 0;
            const bool maySharp = sharpPays && WS_GET(WS_SHARP_RAN) > md.indexBits;
            if (runPlain || (maySharp && __ballot(aliveBits != 0) != 0))
            {
                const u32 aliveBefore = aliveBits;
                const bool use4 = (boundSet == 0);
                float lw[4];
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                    lw[ch] = A.w[ch];
                if (runPlain)
                {
                    u32 CM[4][4];
                    {
                        u32 lpix[16];
                        pixFromLds(lpix);
                        channelMajor(lpix, CM);
                    }
                    // the rest of the block: its raw sums are in LDS since the block bounds
                    auto rest = [&](RawSums &d, const RawSums &a) {
                        d.n = 16 - a.n;
#pragma unroll
                        for (int i = 0; i < 4; i++)
                            d.s[i] = s_scatter[blk][10 + i] - a.s[i];
#pragma unroll
                        for (int i = 0; i < 10; i++)
                            d.p[i] = s_scatter[blk][i] - a.p[i];
                    };
                    // every lane walks its own list: as many rounds as the longest list, not as many as there are slots in use
                    u32 rem = todo;
                    while (__ballot(rem != 0) != 0)
                    {
                        if (rem != 0)
                        {
                            const int k = __ffs((int)rem) - 1;
                            rem &= rem - 1u;
                            const int partition = 4 * k + c;
                            float lb;
                            RawSums s0, s1;
                            if (numSubsets == 2)
                            {
                                maskedRawSumsCM(CM, s_pm2[partition], s1);
                                rest(s0, s1);
                                lb = use4 ? subsetBoundFull<4>(s1, lw, A.delta4) : subsetBoundFull<3>(s1, lw, A.delta3);
                                lb += use4 ? subsetBoundFull<4>(s0, lw, A.delta4) : subsetBoundFull<3>(s0, lw, A.delta3);
                            }
                            else
                            {
                                maskedRawSumsCM(CM, s_pm3[partition] & 0xffffu, s1);
                                rest(s0, s1);
                                lb = subsetBoundFull<3>(s1, lw, A.delta3);
                                maskedRawSumsCM(CM, s_pm3[partition] >> 16, s1);
                                rawSumsSub(s0, s1);
                                lb += subsetBoundFull<3>(s1, lw, A.delta3);
                                lb += subsetBoundFull<3>(s0, lw, A.delta3);
                            }
                            if (!use4)
                                lb += s_static[blk];
                            lbStoreTier2(partition, blk, fmaxf(lb, lbLoad(partition, blk)));
                            BOUND_DUMP(bdEmit(BD_FULL, BD_FORM_CMP, (u32)boundSet, (u32)mode, (u32)numSubsets, 4, (u32)partition, 0, lb, lbLoad(partition, blk), work.err,
                                              lb > work.err, use4 ? 0.0f : s_static[blk]));
                            if (lb > work.err)
                                aliveBits &= ~(1u << k);
                        }
                    }
                }
                u32 rem2 = maySharp ? aliveBits : 0u;
                const bool fourLevels = (md.indexBits == 2);
                const int sharpNeed = (numSubsets * (fourLevels ? CVTT_SHARP_COST4 : CVTT_SHARP_COST8) + md.numP * 4 - 1) / (md.numP * 4);
                // (a wave with fewer candidates than two rounds would have to remove -- noise-like content -- does not start)
                int sharpCand = __popc(rem2);
#pragma unroll
                for (int step = 1; step < 64; step <<= 1)
                    sharpCand += xorLane(sharpCand, step);
                if (maySharp && sharpCand >= 2 * sharpNeed)
                {
                    const u32 aliveMid = aliveBits;
                    const float wSq3 = A.wSqSum3, wSq4 = A.wSqSum3 + A.wSq[3];
                    WS_SET(WS_SHARP_RAN, md.indexBits);
                    WS_SET(WS_BOUND_BITS, WS_GET(WS_BOUND_BITS) < md.indexBits ? WS_GET(WS_BOUND_BITS) : md.indexBits);
                    bool firstRound = true;
                    while (__ballot(rem2 != 0) != 0)
                    {
                        const bool did = rem2 != 0;
                        bool killed = false;
                        if (did)
                        {
                            const int k = __ffs((int)rem2) - 1;
                            rem2 &= rem2 - 1u;
                            const int partition = 4 * k + c;
                            // (subset by subset in a rolled loop: the bound of one subset needs some sixty registers)
                            float lb = 0.0f;
#pragma unroll 1
                            for (int sub = 0; sub < numSubsets; sub++)
                            {
                                const u32 sm = subsetMaskOf(numSubsets, partition, sub);
#ifdef CVTT_BC7_BOUND_DUMP
                                float dUsed[4];
                                const float part1 = use4 ? subsetBoundSharp<4>(&s_pix[blk][0], sm, lw, A.delta4, wSq4, fourLevels, dUsed) : subsetBoundSharp<3>(&s_pix[blk][0], sm, lw, A.delta3, wSq3, fourLevels, dUsed);
                                bdEmit(BD_SHARP, BD_SUBSET, (u32)boundSet, (u32)mode, (u32)numSubsets, (u32)md.indexBits, (u32)partition, (u32)sub, part1, part1, work.err, false,
                                       dUsed[0], dUsed[1], dUsed[2], dUsed[3]);
                                lb += part1;
#else
                                lb += use4 ? subsetBoundSharp<4>(&s_pix[blk][0], sm, lw, A.delta4, wSq4, fourLevels) : subsetBoundSharp<3>(&s_pix[blk][0], sm, lw, A.delta3, wSq3, fourLevels);
#endif
                            }
                            if (!use4)
                                lb += s_static[blk];
                            lbStoreTier2(partition, blk, fmaxf(lb, lbLoad(partition, blk)));
                            BOUND_DUMP(bdEmit(BD_SHARP, BD_FORM_CMP, (u32)boundSet, (u32)mode, (u32)numSubsets, (u32)md.indexBits, (u32)partition, 0, lb, lbLoad(partition, blk),
                                              work.err, lb > work.err, use4 ? 0.0f : s_static[blk]));
                            if (lb > work.err)
                            {
                                aliveBits &= ~(1u << k);
                                killed = true;
                            }
                        }
                        // One round of this loop costs about numSubsets chain passes (0.6 of that without the sort), and a partition
                        // it removes saves a probe: 4 * numP chain lanes for a round and a half.  A round that removes fewer
                        // partitions than it costs ends the loop (the lists of the lanes run out one by one), and when that is
                        // the very first round the wave does not try again in the stages with as many index bits.
                        PROF_STAGE2(stageIter, 0, 1)
                        PROF_STAGE2(stageIter, 1, __popcll(__ballot(did)))
                        PROF_STAGE2(stageIter, 2, __popcll(__ballot(killed)))
                        if (__popcll(__ballot(killed)) < sharpNeed)
                        {
                            if (firstRound)
                                WS_SET(WS_SHARP_NOPAY, md.indexBits);
                            break;
                        }
                        firstRound = false;
                    }
                }
                // content on which these bounds remove nothing (errors dominated by quantisation, not by the fit of
                // a line) does not get them again in the later stages of this wave
                if (runPlain && __ballot(aliveBits != aliveBefore) == 0)
                    WS_SET(WS_T2_NOPAY, md.indexBits);
            }
        }
        // nothing left for any block of the wave (the rule on RGBA noise): on to the next mode
        if (__ballot(aliveBits != 0) == 0)
            continue;
        if (!PT && !HARD && mode == 7 && A.hardCap != 0)
        {
            // A wave with many partitions to search runs for tens of chain passes.  That only matters when it starts
            // near the end of the launch (workgroups are dispatched in order), where it would run on alone: the number
            // of partitions a wave may keep shrinks with the number of waves still to be dispatched after it.
            int cnt = __popc(aliveBits);
            cnt += xorLane(cnt, 1);
            cnt += xorLane(cnt, 2);
            int waveCnt = cnt;
#pragma unroll
            for (int step = 4; step < 64; step <<= 1)
                waveCnt += xorLane(waveCnt, step);
            u32 allowed = (vGrid - vBlock) / A.hardDiv;
            allowed = allowed > A.hardMin ? allowed : A.hardMin;
            // the blocks that make up most of the excess go; an eighth of the allowance each may stay
            if ((u32)waveCnt >= allowed && cnt >= 2 && (u32)cnt >= allowed / 8u)
            {
                u32 slot = 0;
                if (c == 0)
                    slot = atomicAdd(A.hardCount, 1u);
                slot = __shfl(slot, lane & ~3);
                if (slot < A.hardCap)
                {
                    // bit k of sub-lane c is partition 4k + c
                    u64 m = aliveBits;
                    m = (m | (m << 24)) & 0x000000ff000000ffull;
                    m = (m | (m << 12)) & 0x000f000f000f000full;
                    m = (m | (m << 6)) & 0x0303030303030303ull;
                    m = (m | (m << 3)) & 0x1111111111111111ull;
                    m <<= c;
                    u32 lo = (u32)m, hi = (u32)(m >> 32);
                    lo |= xorLane(lo, 1);
                    hi |= xorLane(hi, 1);
                    lo |= xorLane(lo, 2);
                    hi |= xorLane(hi, 2);
                    aliveBits = 0;
                    if (c == 0)
                    {
                        A.hardRec[slot].aliveLo = lo;
                        A.hardRec[slot].aliveHi = hi;
                        s_blkFlags[blk] |= (slot + 1u) << 8; // remembered in LDS until the block's best is final
                    }
                }
            }
        }
        PROF_COUNT(4, __popc(aliveBits))
        PROF_COUNT(5, (c == 0 && valid) ? 1 : 0)
#ifdef CVTT_BC7_PROFILE
        {
            int cntAlive = __popc(aliveBits);
            for (int st = 1; st < 64; st <<= 1) cntAlive += xorLane(cntAlive, st);
            PROF_STAGE(stageIter, 2, cntAlive)
            PROF_STAGE(stageIter, 6, 1)
        }
#endif
        const int itemCap = (numSubsets == 3) ? 21 : 32; // items * subsets <= 64 lanes of the seed pass
        // BC7_RespectPunchThrough couples the 8 blocks of a group in modes 6 and 7 (BC67.cpp:1283-1428): a
        // partition one block wants is searched by its whole group, trial by trial in lock-step
        const bool ptStage = PT && (mode == 6 || mode == 7);
        // Everything else takes its partitions SUBSET BY SUBSET.  The offers of a round (a set of partitions per block, kept
        // as a 64-bit mask) are first PROBED: one unit per partition, its largest subset, searched exactly; the subset's
        // exact error plus the full-dimension bound of the other subset(s) is again a lower bound of the partition's total,
        // and on smooth, photo-like and two-colour content -- where the geometric bounds say little because the errors are
        // quantisation errors -- it rules out 76-99 % of the probed partitions (profiles/r03/bc7_stage_whatif.txt).  Only
        // the survivors are then searched in full (all subsets, payload kept) and committed as before.  The items of a
        // phase are numbered block by block (a block's items are consecutive), in chunks of what the 64 result slots hold.
        const bool staged = !ptStage;
        const bool probing = staged && prune && numSubsets >= 2 && (A.prune & 2u) == 0; // (bit 1 of A.prune: developer knob, probes off)
        const int offerCap = probing ? 64 : itemCap;
        // the subset of a partition that is probed: the one with the most pixels (the first of them)
        auto probeSubOf = [&](int partition) -> int {
            if (numSubsets == 2)
                return __popc((u32)s_pm2[partition]) > 8 ? 1 : 0;
            const u32 m = s_pm3[partition];
            const int n1 = __popc(m & 0xffffu), n2 = __popc(m >> 16), n0 = 16 - n1 - n2;
            return (n2 > n0 && n2 > n1) ? 2 : (n1 > n0) ? 1 : 0;
        };
        // survivors of the probes wait here (per block) until the wave has enough of them for a well-filled full search
        // (CVTT_PEND_MIN partitions) or the stage has nothing left to offer
        u64 pend = 0;
        for (;;)
        {
            // ---- offers.  Pass 0: every block offers its cheapest-bound candidate.  When few
            // blocks offer, the idle lanes take further candidates of the same blocks (they might have been
            // pruned by the first result, but waiting for it would cost a whole round). ----
            REFRESH_LANE();
            int numItems = 0, myCount = 0, maxPasses = 1;
            u64 offerMask = 0; // staged: the partitions this block offers in this round (the same in the four lanes of the quad)
            if (probing)
            {
                // When the partitions the whole wave has left fit one probe phase (64) -- noise-like content, where the bounds
                // leave few -- there is nothing to order and the offer passes are skipped: all of them are probed at once
                // (opaque noise +13 %, near-opaque alpha +22 %).  With more than that the order matters: cheapest bound first, a
                // few per block and round, so that what the first survivors achieve prunes the rest (probing a stage block by
                // block instead measured -12 % on smooth content).
                u64 m = aliveBits; // bit k of sub-lane c is partition 4k + c
                m = (m | (m << 24)) & 0x000000ff000000ffull;
                m = (m | (m << 12)) & 0x000f000f000f000full;
                m = (m | (m << 6)) & 0x0303030303030303ull;
                m = (m | (m << 3)) & 0x1111111111111111ull;
                m <<= c;
                u32 lo = (u32)m, hi = (u32)(m >> 32);
                lo |= xorLane(lo, 1);
                hi |= xorLane(hi, 1);
                lo |= xorLane(lo, 2);
                hi |= xorLane(hi, 2);
                const int kb = __popc(lo) + __popc(hi);
                int allTotal = 0;
#pragma unroll
                for (int b = 0; b < 16; b++)
                    allTotal += __builtin_amdgcn_readlane(kb, 4 * b); // (a scalar: no lane-address register per block to keep alive)
                allTotal = __builtin_amdgcn_readfirstlane(allTotal);
                if (allTotal <= 64)
                {
                    offerMask = ((u64)hi << 32) | lo;
                    aliveBits = 0;
                    numItems = allTotal;
                    maxPasses = 0;
                }
            }
            // Probing stages: every LANE offers the cheapest of the sixteen partitions it looks after (a block offers up to four
            // per pass, nearly its four cheapest), so a full wave fills a probe phase in one pass over the bounds instead of four
            // with a quad-wide argmin each.  The order only steers the pruning, never the result.
            const bool laneOffers = probing;
            for (int pass = 0; pass < maxPasses; pass++)
            {
                // argmin of the bounds still alive (ties: lowest partition), over the quad unless every lane offers for itself
                float pickLb = FLT_MAX;
                int pick = 255;
                for (int k = 0; k * 4 < numPartitions; k++)
                {
                    if ((aliveBits >> k) & 1u)
                    {
                        const float lb = prune ? lbLoad(4 * k + c, blk) : 0.0f;
                        if (lb < pickLb)
                        {
                            pickLb = lb;
                            pick = 4 * k + c;
                        }
                    }
                }
                if (!laneOffers)
                {
#pragma unroll
                    for (int step = 1; step <= 2; step <<= 1)
                    {
                        const float oLb = xorLane(pickLb, step);
                        const int oPick = xorLane(pick, step);
                        const bool take = (oLb < pickLb) || (oLb == pickLb && oPick < pick);
                        pickLb = take ? oLb : pickLb;
                        pick = take ? oPick : pick;
                    }
                }
                bool offer = pick < 64 && !(pickLb > work.err);
#ifdef CVTT_BC7_BOUND_DUMP
                if (prune && pick < 64 && (pick & 3) == c)
                {
                    const float raw = lbLoadRaw(pick, blk);
                    bdEmit(boundSet == 3 ? BD_WHOLE6 : (__builtin_bit_cast(u32, raw) >> 31) ? (WS_GET(WS_SHARP_RAN) < 4 ? BD_SHARP : BD_FULL) : BD_TIER1, BD_RELOAD,
                           (u32)boundSet, (u32)mode, (u32)numSubsets, (u32)md.indexBits, (u32)pick, 0, pickLb, pickLb, work.err, pickLb > work.err, (float)WS_GET(WS_BOUND_BITS), 1.0f);
                }
#endif
                if (!offer)
                    aliveBits = 0; // everything left costs even more
                if (ptStage)
                {
                    // the cheapest offer inside the group becomes the offer of all its blocks
                    if (!offer)
                    {
                        pickLb = FLT_MAX;
                        pick = 255;
                    }
#pragma unroll
                    for (int step = 4; step <= 16; step <<= 1)
                    {
                        const float oLb = xorLane(pickLb, step);
                        const int oPick = xorLane(pick, step);
                        const bool take = (oLb < pickLb) || (oLb == pickLb && oPick < pick);
                        pickLb = take ? oLb : pickLb;
                        pick = take ? oPick : pick;
                    }
                    offer = pick < 64;
                }
                const u64 offers = __ballot(offer && (laneOffers || c == 0));
                const int numOffers = __popcll(offers);
                if (numOffers == 0 || numItems + numOffers > offerCap)
                    break;
                if (pass == 0 && !ptStage)
                {
                    if (laneOffers)
                        maxPasses = numOffers >= 33 ? 1 : numOffers >= 17 ? 2 : numOffers >= 9 ? 4 : numOffers >= 5 ? 8 : 16; // about 64 probes per round
                    else
                        maxPasses = (numOffers <= 1) ? CVTT_SPEC_1 : (numOffers <= 2) ? CVTT_SPEC_2 : (numOffers <= 4) ? CVTT_SPEC_4 : (numOffers <= 8) ? CVTT_SPEC_8 : CVTT_SPEC_16;
                }
                if (offer)
                {
                    if (staged)
                        offerMask |= 1ull << pick;
                    else
                    {
                        const int item = numItems + __popcll(offers & ((1ull << (lane & ~3)) - 1ull));
                        if (c == 0)
                        {
                            s_item[item] = (u32)blk | ((u32)pick << 8);
                            s_myItems[PT ? blk : 0][pass] = (uint8_t)item;
                        }
                    }
                    if ((pick & 3) == c)
                        aliveBits &= ~(1u << (pick >> 2));
                    myCount = pass + 1;
                }
                numItems += numOffers;
            }
            if (laneOffers)
            {
                u32 lo = (u32)offerMask, hi = (u32)(offerMask >> 32);
                lo |= xorLane(lo, 1);
                hi |= xorLane(hi, 1);
                lo |= xorLane(lo, 2);
                hi |= xorLane(hi, 2);
                offerMask = ((u64)hi << 32) | lo;
            }
            PROF_MARK(8)
            const bool flush = (numItems == 0); // nothing left to offer: the waiting survivors are searched, then the stage ends
            if (flush && __ballot(pend != 0) == 0)
                break;
            PROF_STAGE(stageIter, 3, 1)
            bool isProbe = probing && !flush;
            u64 curMask = offerMask; // staged: this block's partitions of the current phase
            if (!isProbe)
            {
                curMask |= pend;
                pend = 0;
            }
            int chunkLo = 0;
            for (;;) // phases of the round: [probe,] then the full search of the survivors, chunk by chunk
            {
            PROF_MARK(14)
            REFRESH_LANE();
            int iLo = 0, iHi = 0, phaseTotal = numItems;
            if (staged)
            {
                // number the items block by block and write this chunk's part of the list
                const int kb = __popcll(curMask);
                int base = 0;
                phaseTotal = 0;
#pragma unroll
                for (int b = 0; b < 16; b++)
                {
                    const int o = __builtin_amdgcn_readlane(kb, 4 * b);
                    base += (b < blk) ? o : 0;
                    phaseTotal += o;
                }
                phaseTotal = __builtin_amdgcn_readfirstlane(phaseTotal);
                const int cap = isProbe ? 64 : itemCap;
                numItems = phaseTotal - chunkLo < cap ? phaseTotal - chunkLo : cap;
                iLo = base - chunkLo;
                iHi = iLo + kb;
                iLo = iLo < 0 ? 0 : (iLo > numItems ? numItems : iLo);
                iHi = iHi < 0 ? 0 : (iHi > numItems ? numItems : iHi);
                // sub-lane c files the partitions 16c .. 16c+15 of the block's mask
                u32 part = (u32)(curMask >> (16 * c)) & 0xffffu;
                int rnk = base - chunkLo + __popcll(curMask & ((1ull << (16 * c)) - 1ull));
                while (part)
                {
                    const int bit = __ffs((int)part) - 1;
                    part &= part - 1u;
                    if (rnk >= 0 && rnk < numItems)
                        s_item[rnk] = (u32)blk | ((u32)(16 * c + bit) << 8);
                    rnk++;
                }
            }
            const int numUnits = isProbe ? numItems : numItems * numSubsets;
            PROF_STAGE(stageIter, isProbe ? 7 : 1, numUnits)
            __syncthreads();

            // ---- PCA seed search: lane l takes unit l = (item, subset) ----
            // The chain lanes of a batch walk the member pixels of their subsets in lock-step, i.e. as many steps as the
            // largest subset of the batch has pixels: the units are therefore filed in ascending order of their pixel
            // counts (a counting sort on ballots), so that a batch holds subsets of (nearly) one size.  Results are routed
            // by UnitRec::slot, so the order of the units is free.  (The punch-through replay indexes units by item.)
            int unitPos = lane;
            {
                int cnt = 0;
                if (lane < numUnits && numSubsets >= 2 && !ptStage)
                {
                    const int item = isProbe ? lane : (numSubsets == 2) ? (lane >> 1) : (lane / 3);
                    const int upart = (int)(s_item[item] >> 8);
                    const int sub = isProbe ? probeSubOf(upart) : lane - item * numSubsets;
                    cnt = __popc(subsetMaskOf(numSubsets, upart, sub));
                }
                if (numSubsets >= 2 && !ptStage)
                {
                    int base = 0;
                    for (int v = 1; v < 16; v++)
                    {
                        const u64 m = __ballot(cnt == v);
                        if (m == 0)
                            continue;
                        if (cnt == v)
                            unitPos = base + (int)__builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
                        base += __popcll(m);
                    }
                }
            }
            PROF_MARK(9)
            REFRESH_LANE();
            if (lane < numUnits)
            {
                const int item = (isProbe || numSubsets == 1) ? lane : (numSubsets == 2) ? (lane >> 1) : (lane / 3);
                const u32 it = s_item[item];
                const int ublk = (int)(it & 255u), upart = (int)(it >> 8);
                const int sub = isProbe ? probeSubOf(upart) : lane - item * numSubsets;
                int shape = 0;
                if (numSubsets == 2)
                    shape = T->shapes2[upart][sub];
                else if (numSubsets == 3)
                    shape = T->shapes3[upart][sub];
                const u32 uMask = subsetMaskOf(numSubsets, upart, sub);
                int seeds = isRGB ? plan->seedPointsForShapeRGB[shape] : plan->seedPointsForShapeRGBA[shape];
                if (seeds > 4)
                    seeds = 4;
                const bool rgbListed = ((dplan->rgbListed[shape >> 5] >> (shape & 31)) & 1u) != 0;
                const bool rgbaListed = isRGB ? true : (((dplan->rgbaListed[shape >> 5] >> (shape & 31)) & 1u) != 0);
                const bool uWantPCA4 = (s_blkFlags[ublk] & 1u) != 0;
                const bool wanted = seeds > 0;
                // which PCA does this unit need?  (BC67.cpp:1085-1144; unlisted shapes keep zero seeds)
                const bool do4 = wanted && !isRGB && uWantPCA4 && rgbaListed;
                const bool do3 = wanted && rgbListed && (isRGB || (!uWantPCA4 && rgbaListed));
                const bool expandAlpha = !isRGB && wanted && !uWantPCA4 && rgbaListed;
                Unfinished uu;
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                    uu.base[ch] = uu.offset[ch] = 0.0f;
                const u32 *lp = &s_pix[ublk][0];
                float vsum[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // the refiner's m_v (UnitRec::vs); the PCA's first pass forms the same sums
                if (do3)
                {
                    Unfinished u3;
                    pcaEndpointsLDS<3>(lp, uMask, A.w, u3, vsum);
#pragma unroll
                    for (int ch = 0; ch < 3; ch++)
                    {
                        uu.base[ch] = u3.base[ch];
                        uu.offset[ch] = u3.offset[ch];
                    }
                }
                if (expandAlpha)
                {
                    uu.base[3] = 255.0f; // ExpandTo<4>(255), UnfinishedEndpoints.h:93-114
                    uu.offset[3] = 0.0f;
                }
                if (do4)
                    pcaEndpointsLDS<4>(lp, uMask, A.w, uu, vsum);
                if (wanted && !do4)
                {
                    // no four-channel pass ran: alpha of an RGBA mode whose seeds come from the RGB pass, or every channel
                    // of a shape the plan does not list (zero seeds, but its chains still run)
#pragma unroll
                    for (int ch = 0; ch < 4; ch++)
                        if (ch == 3 ? !isRGB : !do3)
                        {
                            float a = 0.0f;
#pragma unroll
                            for (int px = 0; px < 16; px++)
                                if ((uMask >> px) & 1u)
                                    a = a + byteF(lp[px], ch) * A.w[ch];
                            vsum[ch] = a;
                        }
                }
                UnitRec &r = s_unit[unitPos];
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                {
                    r.base[ch] = uu.base[ch];
                    r.offset[ch] = uu.offset[ch];
                }
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                    r.vs[ch] = vsum[ch];
                // where the unit's result goes: a probe's by item, a full search's by (item, subset)
                r.packed = uMask | ((u32)(seeds < 0 ? 0 : seeds) << 16) | ((u32)ublk << 20) | ((u32)(isProbe ? item : item * numSubsets + sub) << 24);
                float scErr = FLT_MAX;
                if ((A.flags & CVTTMI_FLAG_BC7_TRY_SINGLE_COLOR) && seeds > 0)
                {
                    // BC67.cpp:1436-1570 + 940-1040.  With the reference's AndNot operand order no
                    // single-colour table entry is ever taken (finite weights), so what reaches the
                    // error test is endpoints (0,0,0[,255]) with index 0 for every pixel.
                    u32 e[4] = {0, 0, 0, 0}, st = 0;
#pragma unroll
                    for (int px = 0; px < 16; px++)
                        if ((uMask >> px) & 1u)
                        {
                            const u32 pk = lp[px];
                            e[0] = (u32)mad24(byteI(pk, 0), byteI(pk, 0), (int)e[0]);
                            e[1] = (u32)mad24(byteI(pk, 1), byteI(pk, 1), (int)e[1]);
                            e[2] = (u32)mad24(byteI(pk, 2), byteI(pk, 2), (int)e[2]);
                            const int d = 255 - byteI(pk, 3);
                            if (isRGB)
                                st = (u32)mad24(d, d, (int)st);
                            else
                                e[3] = (u32)mad24(d, d, (int)e[3]);
                        }
                    const bool uniformErr = (A.flags & CVTTMI_FLAG_UNIFORM) != 0;
                    if (uniformErr)
                        scErr = (float)(int)(e[0] + e[1] + e[2] + e[3]);
                    else
                    {
                        scErr = (float)(int)e[0] * A.wSq[0];
                        scErr = scErr + (float)(int)e[1] * A.wSq[1];
                        scErr = scErr + (float)(int)e[2] * A.wSq[2];
                        scErr = scErr + (float)(int)e[3] * A.wSq[3];
                    }
                    if (isRGB)
                        scErr = scErr + (uniformErr ? (float)(int)st : (float)(int)st * A.wSq[3]);
                }
                r.scErr = scErr;
                {
                    u32 lo = 0, hi = 0;
                    int k = 0;
#pragma unroll
                    for (int px = 0; px < 16; px++)
                        if ((uMask >> px) & 1u)
                        {
                            if (k < 8)
                                lo |= (u32)px << (4 * k);
                            else
                                hi |= (u32)px << (4 * k - 32);
                            k++;
                        }
                    r.listLo = lo;
                    r.listHi = hi;
                }
            }
            __syncthreads();
            PROF_MARK(10)

            REFRESH_LANE();
            // ---- probes with two refine rounds (the default): round 1 only once per distinct set of end points.  The four seed
            // points of a (unit, p-bits) often refine to the same end points, or to end points round 0 has already tried
            // (24-47 % of all chain rounds on smooth / photo-like / two-colour content, tools/bc7_dup_profile.py) -- the same
            // end points on the same pixels give the same error, and a probe wants nothing but the minimum.  So a batch runs
            // round 0 of its 64 chains, the chains whose round-1 end points are new file them (unit, end points) in a ring in
            // LDS (the payload words of s_res, idle during a probe), and whenever 64 are waiting one batch runs them; the
            // minima are taken with ds_min_u32 on the error bits (errors are >= 0). ----
            const bool dedup = isProbe && numRefine == 2 && (A.prune & 4u) == 0;
            if (dedup)
            {
                constexpr int kRing = 85; // items of three dwords in words 1..4 of the 64 result rows
                auto ringWord = [&](int item, int j) -> u32 * {
                    const int flat = item * 3 + j;
                    return &s_res[flat >> 2][1 + (flat & 3)];
                };
                if (lane < numUnits)
                {
                    const UnitRec &ru = s_unit[lane];
                    s_res[ru.slot()][0] = __builtin_bit_cast(u32, ru.scErr); // the single-colour try (FLT_MAX when there is none)
                }
                __syncthreads();
                int ringHead = 0, ringCount = 0;
                auto runRound1 = [&](int n) {
                    // lane l < n takes the l-th waiting item
                    const bool have = lane < n;
                    int it = ringHead + lane;
                    it -= it >= kRing ? kRing : 0;
                    const u32 w0 = have ? *ringWord(it, 0) : 0u;
                    ChainSplit sp;
                    sp.firstRound = 1;
                    sp.endRound = 2;
                    sp.ep0 = have ? *ringWord(it, 1) : 0u;
                    sp.ep1 = have ? *ringWord(it, 2) : 0u;
                    sp.r0ep0 = sp.r0ep1 = 0;
                    const UnitRec &r = s_unit[w0 & 63u];
                    const u32 uMask = r.mask();
                    int maxCount = have ? __popc(uMask) : 0;
#pragma unroll
                    for (int step = 1; step < 64; step <<= 1)
                    {
                        const int o = xorLane(maxCount, step);
                        maxCount = o > maxCount ? o : maxCount;
                    }
                    maxCount = __builtin_amdgcn_readfirstlane(maxCount);
                    Unfinished uu;
#pragma unroll
                    for (int ch = 0; ch < 4; ch++)
                        uu.base[ch] = uu.offset[ch] = 0.0f; // not used: the end points come with the item
                    const float uvs[4] = {0.0f, 0.0f, 0.0f, 0.0f}; // the last round refines nothing
                    const u64 uList = ((u64)r.listHi << 32) | r.listLo;
                    ShapeBest b;
                    if (isRGB)
                        evalChain<3, FAST, false>(&s_pix[r.blk()][0], uMask, uList, maxCount, md, uu, 0, 0, have, A, T, numRefine, b, uvs, false, nullptr, -1, nullptr, &sp);
                    else
                        evalChain<4, FAST, false>(&s_pix[r.blk()][0], uMask, uList, maxCount, md, uu, 0, 0, have, A, T, numRefine, b, uvs, false, nullptr, -1, nullptr, &sp);
                    if (have)
                        atomicMin(&s_res[r.slot()][0], __builtin_bit_cast(u32, b.err));
                    ringHead += n;
                    ringHead -= ringHead >= kRing ? kRing : 0;
                    ringCount -= n;
                    __syncthreads();
                };
                for (int u0 = 0; u0 < numUnits; u0 += UPB)
                {
                    const int unit = u0 + lane / CP;
                    const int chain = lane & (CP - 1);
                    const bool inRange = unit < numUnits;
                    const UnitRec &r = s_unit[inRange ? unit : 0];
                    const int tweak = chain & 3, pIter = chain >> 2;
                    const u32 uMask = r.mask();
                    const bool active = inRange && tweak < r.numTweak();
                    int maxCount = active ? __popc(uMask) : 0;
#pragma unroll
                    for (int step = 1; step < 64; step <<= 1)
                    {
                        const int o = xorLane(maxCount, step);
                        maxCount = o > maxCount ? o : maxCount;
                    }
                    maxCount = __builtin_amdgcn_readfirstlane(maxCount);
                    Unfinished uu;
#pragma unroll
                    for (int ch = 0; ch < 4; ch++)
                    {
                        uu.base[ch] = r.base[ch];
                        uu.offset[ch] = r.offset[ch];
                    }
                    const float uvs[4] = {r.vs[0], r.vs[1], r.vs[2], r.vs[3]};
                    const u64 uList = ((u64)r.listHi << 32) | r.listLo;
                    PROF_STAGE(stageIter, 0, 1)
                    PROF_STAGE_LANES(stageIter, 5, active)
                    ChainSplit sp;
                    sp.firstRound = 0;
                    sp.endRound = 1;
                    sp.ep0 = sp.ep1 = sp.r0ep0 = sp.r0ep1 = 0;
                    ShapeBest b;
                    if (isRGB)
                        evalChain<3, FAST, false>(&s_pix[r.blk()][0], uMask, uList, maxCount, md, uu, pIter, tweak, active, A, T, numRefine, b, uvs, false, nullptr, -1, nullptr, &sp);
                    else
                        evalChain<4, FAST, false>(&s_pix[r.blk()][0], uMask, uList, maxCount, md, uu, pIter, tweak, active, A, T, numRefine, b, uvs, false, nullptr, -1, nullptr, &sp);
                    if (active)
                        atomicMin(&s_res[r.slot()][0], __builtin_bit_cast(u32, b.err));
                    // is my round 1 new?  Not if a lower seed point of my (unit, p-bits) goes to the same end points, and not
                    // if some seed point of it has just tried them in round 0
                    bool needed = active;
#pragma unroll
                    for (int o = 0; o < 4; o++)
                    {
                        const int src = (lane & ~3) | o;
                        const bool oAct = __shfl((int)active, src) != 0;
                        const u32 n0 = __shfl(sp.ep0, src), n1 = __shfl(sp.ep1, src);
                        const u32 q0 = __shfl(sp.r0ep0, src), q1 = __shfl(sp.r0ep1, src);
                        if (oAct && o < (lane & 3) && n0 == sp.ep0 && n1 == sp.ep1)
                            needed = false;
                        if (oAct && q0 == sp.ep0 && q1 == sp.ep1)
                            needed = false;
                    }
                    const u64 nm = __ballot(needed);
                    const int nNew = __popcll(nm);
                    // room for them?  (only when the ring is nearly full: a short batch then)
                    if (ringCount + nNew > kRing)
                        runRound1(ringCount < 64 ? ringCount : 64);
                    if (needed)
                    {
                        int it = ringHead + ringCount + (int)__builtin_amdgcn_mbcnt_hi((u32)(nm >> 32), __builtin_amdgcn_mbcnt_lo((u32)nm, 0u));
                        it -= it >= kRing ? kRing : 0;
                        *ringWord(it, 0) = (u32)unit;
                        *ringWord(it, 1) = sp.ep0;
                        *ringWord(it, 2) = sp.ep1;
                    }
                    ringCount += nNew;
                    __syncthreads();
                    while (ringCount >= 64)
                        runRound1(64);
                }
                while (ringCount > 0)
                    runRound1(ringCount < 64 ? ringCount : 64);
            }
            else
            // ---- chains: lane l of a batch = (unit l / CP, p-bits (l % CP) / 4, seed point l % 4) ----
            for (int u0 = 0; u0 < numUnits; u0 += UPB)
            {
                const int unit = u0 + lane / CP;
                const int chain = lane & (CP - 1);
                const bool inRange = unit < numUnits;
                const UnitRec &r = s_unit[inRange ? unit : 0];
                const int tweak = chain & 3, pIter = chain >> 2;
                const u32 uMask = r.mask();
                const bool active = inRange && tweak < r.numTweak();
                int maxCount = active ? __popc(uMask) : 0;
#pragma unroll
                for (int step = 1; step < 64; step <<= 1)
                {
                    const int o = xorLane(maxCount, step);
                    maxCount = o > maxCount ? o : maxCount;
                }
                maxCount = __builtin_amdgcn_readfirstlane(maxCount);
                Unfinished uu;
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                {
                    uu.base[ch] = r.base[ch];
                    uu.offset[ch] = r.offset[ch];
                }
                const u32 *lp = &s_pix[r.blk()][0];
                const float uvs[4] = {r.vs[0], r.vs[1], r.vs[2], r.vs[3]};
                const u64 uList = ((u64)r.listHi << 32) | r.listLo;
                PROF_COUNT(2, 64)
                PROF_COUNT(3, __popcll(__ballot(active)))
                PROF_STAGE(stageIter, 0, 1)
                PROF_STAGE_LANES(stageIter, 5, active)
                ShapeBest b;
                if (ptStage)
                {
                    // record every trial; the lock-step commit rule is applied below
                    if (PT)
                        evalChain<4, FAST, true>(lp, uMask, uList, maxCount, md, uu, pIter, tweak, active, A, T, numRefine, b, uvs, true,
                                                 trialHbm ? nullptr : &s_trialErr[((inRange ? unit : 0) * 16 + chain) * numRefine], -1,
                                                 trialHbm ? trialHbm + ((inRange ? unit : 0) * 16 + chain) * numRefine : nullptr);
                    continue;
                }
                if (isRGB)
                    evalChain<3, FAST, false>(lp, uMask, uList, maxCount, md, uu, pIter, tweak, active, A, T, numRefine, b, uvs, !isProbe);
                else
                    evalChain<4, FAST, false>(lp, uMask, uList, maxCount, md, uu, pIter, tweak, active, A, T, numRefine, b, uvs, !isProbe);
                groupArgminBroadcast(b, lane, CP);
                if (inRange && chain == 0)
                {
                    if (r.scErr < b.err)
                    {
                        // the single-colour try comes after every chain of the shape (strict '<')
                        b.err = r.scErr;
                        b.ep0 = b.ep1 = isRGB ? 0u : 0xff000000u;
                        b.idxLo = b.idxHi = 0;
                    }
                    // with no seed points the shape keeps its reset error FLT_MAX (BC67.cpp:1228-1242)
                    u32 *dst = &s_res[r.slot()][0];
                    dst[0] = __builtin_bit_cast(u32, b.err);
                    dst[1] = b.ep0;
                    dst[2] = b.ep1;
                    dst[3] = b.idxLo;
                    dst[4] = b.idxHi;
                }
            }
            __syncthreads();
            if (isProbe) { PROF_MARK(11) } else { PROF_MARK(13) }
            REFRESH_LANE();

            if (isProbe)
            {
                // ---- which of the probed partitions can still win?  Exact error of the probed subset + full-dimension
                // bound of the other subset(s) <= the partition's total in the reference: for two subsets the total is the
                // float sum of the same two kinds of terms (rounding is monotone); for three the association differs, which
                // the factor below covers (the total is >= the real sum * (1 - 2u), this sum <= the real one * (1 + 2u)).
                // Sub-lane c takes the block's items c, c + 4, ... ----
                u64 surv = 0;
                if (__ballot(iLo + c < iHi) != 0)
                {
                    const bool use4 = (boundSet == 0);
                    const float lwf[4] = {A.w[0], A.w[1], A.w[2], A.w[3]};
                    {
                        u32 CMf[4][4];
                        {
                            u32 lpix[16];
                            pixFromLds(lpix);
                            channelMajor(lpix, CMf);
                        }
                        for (int i = iLo + c; __ballot(i < iHi) != 0; i += 4)
                        {
                            if (i < iHi)
                            {
                                const int partition = (int)(s_item[i] >> 8);
                                const float eProbed = __builtin_bit_cast(float, s_res[i][0]);
                                const int ps = probeSubOf(partition);
                                float lbRest = 0.0f;
                                for (int sub = 0; sub < numSubsets; sub++)
                                {
                                    if (sub == ps)
                                        continue;
                                    RawSums rs;
                                    maskedRawSumsCM(CMf, subsetMaskOf(numSubsets, partition, sub), rs);
                                    lbRest += use4 ? subsetBoundFull<4>(rs, lwf, A.delta4) : subsetBoundFull<3>(rs, lwf, A.delta3);
                                }
                                const float lbTotal = (eProbed + lbRest) * 0.9999995f;
                                BOUND_DUMP(bdEmit(BD_PROBE_FULL, BD_FORM_CMP, (u32)boundSet, (u32)mode, (u32)numSubsets, (u32)md.indexBits, (u32)partition, (u32)ps, lbTotal, lbTotal,
                                                  work.err, lbTotal > work.err, eProbed, lbRest));
                                if (!(lbTotal > work.err))
                                    surv |= 1ull << partition;
                            }
                        }
                    }
                    // what the plain bound of the rest leaves gets the sharper one (in a wave where that one pays: see the second tier)
                    // (a partition it removes saves a full search -- numSubsets * 4 numP chain lanes for two rounds --, a round of
                    // this loop costs about numSubsets - 1 chain passes: it runs as long as a round removes what it costs, and a
                    // wave gives it up after CVTT_FILTER_STRIKES calls in a row whose first round did not)
                    const int filterNeed = ((numSubsets - 1) * (md.indexBits == 2 ? 40 : 26) + numSubsets * md.numP * 4 - 1) / (numSubsets * md.numP * 4);
                    // (surv is per lane here: sub-lane c has filed the items c, c + 4, ... of its block)
                    int filterCand = __popcll(surv);
#pragma unroll
                    for (int step = 1; step < 64; step <<= 1)
                        filterCand += xorLane(filterCand, step);
                    if (WS_GET(WS_STRIKES) < CVTT_FILTER_STRIKES && filterCand >= 2 * filterNeed)
                    {
                        bool firstRound = true;
                        for (int i = iLo + c; __ballot(i < iHi) != 0; i += 4)
                        {
                            const int partition = i < iHi ? (int)(s_item[i] >> 8) : 0;
                            bool killed = false;
                            if (i < iHi && ((surv >> partition) & 1ull))
                            {
                                const float eProbed = __builtin_bit_cast(float, s_res[i][0]);
                                const int ps = probeSubOf(partition);
                                float lbRest = 0.0f;
#pragma unroll 1
                                for (int sub = 0; sub < numSubsets; sub++)
                                {
                                    if (sub == ps)
                                        continue;
                                    const u32 sm = subsetMaskOf(numSubsets, partition, sub);
#ifdef CVTT_BC7_BOUND_DUMP
                                    float dUsed[4];
                                    const float part1 = use4 ? subsetBoundSharp<4>(&s_pix[blk][0], sm, lwf, A.delta4, A.wSqSum3 + A.wSq[3], md.indexBits == 2, dUsed)
                                                             : subsetBoundSharp<3>(&s_pix[blk][0], sm, lwf, A.delta3, A.wSqSum3, md.indexBits == 2, dUsed);
                                    bdEmit(BD_PROBE_SHARP, BD_SUBSET, (u32)boundSet, (u32)mode, (u32)numSubsets, (u32)md.indexBits, (u32)partition, (u32)sub, part1, part1, work.err, false,
                                           dUsed[0], dUsed[1], dUsed[2], dUsed[3]);
                                    lbRest += part1;
#else
                                    lbRest += use4 ? subsetBoundSharp<4>(&s_pix[blk][0], sm, lwf, A.delta4, A.wSqSum3 + A.wSq[3], md.indexBits == 2)
                                                   : subsetBoundSharp<3>(&s_pix[blk][0], sm, lwf, A.delta3, A.wSqSum3, md.indexBits == 2);
#endif
                                }
                                const float lbTotal = (eProbed + lbRest) * 0.9999995f;
                                BOUND_DUMP(bdEmit(BD_PROBE_SHARP, BD_FORM_CMP, (u32)boundSet, (u32)mode, (u32)numSubsets, (u32)md.indexBits, (u32)partition, (u32)ps, lbTotal, lbTotal,
                                                  work.err, lbTotal > work.err, eProbed, lbRest));
                                if (lbTotal > work.err)
                                {
                                    surv &= ~(1ull << partition);
                                    killed = true;
                                }
                            }
                            PROF_STAGE2(stageIter, 3, 1)
                            PROF_STAGE2(stageIter, 4, __popcll(__ballot(i < iHi && ((surv >> partition) & 1ull))) + __popcll(__ballot(killed)))
                            PROF_STAGE2(stageIter, 5, __popcll(__ballot(killed)))
                            if (__popcll(__ballot(killed)) < filterNeed)
                            {
                                if (firstRound)
                                    WS_SET(WS_STRIKES, WS_GET(WS_STRIKES) + 1);
                                break;
                            }
                            WS_SET(WS_STRIKES, 0);
                            firstRound = false;
                        }
                    }
                }
                {
                    u32 lo = (u32)surv, hi = (u32)(surv >> 32);
                    lo |= xorLane(lo, 1);
                    hi |= xorLane(hi, 1);
                    lo |= xorLane(lo, 2);
                    hi |= xorLane(hi, 2);
                    surv = ((u64)hi << 32) | lo;
                }
                pend |= surv;
                int pendTotal = 0;
                {
                    const int kb = __popcll(pend);
#pragma unroll
                    for (int b = 0; b < 16; b++)
                        pendTotal += __builtin_amdgcn_readlane(kb, 4 * b);
                    pendTotal = __builtin_amdgcn_readfirstlane(pendTotal);
                }
                __syncthreads(); // everybody has read its items before the next list is written
                PROF_MARK(12)
                if (pendTotal < CVTT_PEND_MIN)
                    break; // they wait for more
                curMask = pend;
                pend = 0;
                isProbe = false;
                chunkLo = 0;
                continue;
            }

            if (PT && ptStage)
            {
                __syncthreads();
                // ---- the reference's commit rule, trial by trial, for the 8 blocks of a group together
                // (BC67.cpp:1283-1428): lane = (group of the round, subset, block of the group) ----
                const int perGroup = 8 * numSubsets;
                const int gi = lane / perGroup, sub = (lane - gi * perGroup) >> 3, l8 = lane & 7;
                const int item = gi * 8 + l8;
                const bool scanActive = item < numItems && lane < (numItems / 8) * perGroup;
                const int unit = scanActive ? item * numSubsets + sub : 0;
                const UnitRec &r = s_unit[unit];
                const u32 bf = s_blkFlags[r.blk()];
                const bool isPT = (bf & 2u) != 0, nonZeroA = (bf & 4u) != 0, nonMaxA = (bf & 8u) != 0;
                const int slice = lane & ~7;
                float held = FLT_MAX; // shapeBestError
                int last = -1;        // the trial whose result the shape holds
                for (int pI = 0; pI < 4; pI++)
                {
                    const bool invalid = scanActive && ((pI == 0) ? (isPT && nonZeroA) : (pI == 3) ? (isPT && nonMaxA) : isPT);
                    const u32 invSlice = (u32)(__ballot(invalid) >> slice) & 0xffu;
                    const bool allInvalid = invSlice == 0xffu;
                    const bool needCheck = invSlice != 0;
                    for (int tw = 0; tw < 4; tw++)
                        for (int rf = 0; rf < numRefine; rf++)
                        {
                            const int t = (pI * 4 + tw) * numRefine + rf;
                            const bool run = scanActive && !allInvalid && tw < r.numTweak();
                            const float e = run ? (trialHbm ? trialHbm[unit * 16 * numRefine + t] : s_trialErr[unit * 16 * numRefine + t]) : FLT_MAX;
                            const bool better = run && e < held;
                            const bool anyBetter = ((u32)(__ballot(better) >> slice) & 0xffu) != 0;
                            bool commit = better;
                            if (needCheck)
                            {
                                // AndNot(punchThroughInvalid, better) = invalid & ~better (ParallelMath.h:900-905)
                                commit = run && invalid && !better;
                                if (((u32)(__ballot(commit) >> slice) & 0xffu) == 0)
                                    commit = false;
                            }
                            if (anyBetter && commit)
                            {
                                held = e;
                                last = t;
                            }
                        }
                }
                // the payload of the held trial: run that chain again up to its round
                const bool have = scanActive && last >= 0;
                const int hChain = have ? last / numRefine : 0, hRound = have ? last - hChain * numRefine : 0;
                int maxCount = have ? __popc(r.mask()) : 0;
#pragma unroll
                for (int step = 1; step < 64; step <<= 1)
                {
                    const int o = xorLane(maxCount, step);
                    maxCount = o > maxCount ? o : maxCount;
                }
                maxCount = __builtin_amdgcn_readfirstlane(maxCount);
                Unfinished uu;
#pragma unroll
                for (int ch = 0; ch < 4; ch++)
                {
                    uu.base[ch] = r.base[ch];
                    uu.offset[ch] = r.offset[ch];
                }
                ShapeBest b;
                const float uvs[4] = {r.vs[0], r.vs[1], r.vs[2], r.vs[3]};
                evalChain<4, FAST, true>(&s_pix[r.blk()][0], r.mask(), ((u64)r.listHi << 32) | r.listLo, maxCount, md, uu, hChain >> 2, hChain & 3, have, A, T, numRefine, b, uvs,
                                         true, nullptr, hRound);
                if (scanActive)
                {
                    if (!have)
                    {
                        b.err = FLT_MAX;
                        b.ep0 = b.ep1 = b.idxLo = b.idxHi = 0;
                    }
                    if (r.scErr < b.err)
                    {
                        b.err = r.scErr;
                        b.ep0 = b.ep1 = 0xff000000u;
                        b.idxLo = b.idxHi = 0;
                    }
                    u32 *dst = &s_res[r.slot()][0];
                    dst[0] = __builtin_bit_cast(u32, b.err);
                    dst[1] = b.ep0;
                    dst[2] = b.ep1;
                    dst[3] = b.idxLo;
                    dst[4] = b.idxHi;
                }
            }
            REFRESH_LANE();
            // ---- every offering block adds up the subsets of its items and commits ----
            for (int j = 0; j < 64; j++)
            {
                const bool mine = staged ? (iLo + j < iHi) : (j < myCount);
                if (__ballot(mine) == 0)
                    break;
                if (mine)
                {
                    const int item = staged ? iLo + j : (int)s_myItems[PT ? blk : 0][j];
                    const int partition = (int)(s_item[item] >> 8);
                    float totalError = 0.0f;
                    u32 pe[3][2] = {{0, 0}, {0, 0}, {0, 0}};
                    // the index sets come compact (member i of a subset in bits [4i, 4i + 4)): subset after subset, still
                    // compact -- expandIndexes sorts them to their pixels when the block is packed
                    u64 pIdx = 0;
                    int nibbles = 0;
                    for (int sub = 0; sub < numSubsets; sub++)
                    {
                        const u32 *src = &s_res[item * numSubsets + sub][0];
                        totalError = totalError + __builtin_bit_cast(float, src[0]);
                        const u32 e0 = src[1], e1 = src[2];
                        if (sub == 0) { pe[0][0] = e0; pe[0][1] = e1; }
                        else if (sub == 1) { pe[1][0] = e0; pe[1][1] = e1; }
                        else { pe[2][0] = e0; pe[2][1] = e1; }
                        const u64 part = ((u64)src[4] << 32) | src[3];
                        pIdx |= nibbles < 16 ? part << (4 * nibbles) : 0ull;
                        nibbles += __popc(subsetMaskOf(numSubsets, partition, sub));
                    }
                    const u32 pIdxLo = (u32)pIdx, pIdxHi = (u32)(pIdx >> 32);
                    const int seq = stage * 64 + partition;
                    bool mayTake = laneRuns;
                    if (ptStage && mode == 7 && anyBlockHasAlpha && !blockHasNonMaxAlpha && ((mode7RGB >> partition) & 1ull) == 0)
                        mayTake = false; // searched for the group's sake only (BC67.cpp:1625-1635)
                    PROF_STAGE_LANES(stageIter, 4, c == 0 && mayTake && (totalError < work.err || (totalError == work.err && seq < workSeq)))
                    if (mayTake && (totalError < work.err || (totalError == work.err && seq < workSeq)))
                    {
                        work.err = totalError;
                        workSeq = seq;
                        workPay0 = (c == 0) ? pe[0][0] : (c == 1) ? pe[1][0] : (c == 2) ? pe[2][0] : pIdxLo;
                        workPay1 = (c == 0) ? pe[0][1] : (c == 1) ? pe[1][1] : (c == 2) ? pe[2][1] : pIdxHi;
                    }
                }
            }
            if (!staged)
                break;
            chunkLo += itemCap;
            if (chunkLo >= phaseTotal)
                break;
            __syncthreads(); // the commits have read this chunk's items and results
            } // phases of the round
            PROF_MARK(14)
            if (flush)
                break;
        }
    }

    // ===================== fix-ups + bit packing (reference BC67.cpp:2003-2203) ==========
    REFRESH_LANE();
    {
        // the winner: seq = stage * 64 + partition for the single-plane modes (stages 0..5 = modes 0, 1, 2, 3, 6, 7),
        // 384 + rotation * 2 + index selector for mode 4, 392 + rotation for mode 5; nothing committed: mode 0, all zero
        WorkState packed;
        {
            const int sq = workSeq < 0 ? 0 : workSeq;
            const int cfg = sq - 384;
            const int stage = sq >> 6;
            packed.mode = (sq >= 392) ? 5 : (sq >= 384) ? 4 : (stage >= 4) ? stage + 2 : stage;
            packed.partOrIS = (sq >= 392) ? 0 : (sq >= 384) ? (cfg & 1) : (sq & 63);
            packed.rotation = (sq >= 392) ? cfg - 8 : (sq >= 384) ? (cfg >> 1) : 0;
            const int q = lane & ~3;
            packed.ep[0][0] = __shfl(workPay0, q);
            packed.ep[0][1] = __shfl(workPay1, q);
            packed.ep[1][0] = __shfl(workPay0, q | 1);
            packed.ep[1][1] = __shfl(workPay1, q | 1);
            packed.ep[2][0] = __shfl(workPay0, q | 2);
            packed.ep[2][1] = __shfl(workPay1, q | 2);
            packed.idxLo = __shfl(workPay0, q | 3);
            packed.idxHi = __shfl(workPay1, q | 3);
            packed.idx2Lo = packed.idx2Hi = 0;
            if (packed.mode < 4 || packed.mode == 7)
            {
                // single-plane results carry their indexes compact, subset after subset in member order: sort them to their
                // pixels (sub-lane c places pixels 4c .. 4c + 3; mode 6 is one subset of 16; modes 4 / 5 keep the layout of their
                // search, dualIndexSlot, which packDualPlane reads)
                const int p = packed.partOrIS;
                const bool three = (packed.mode == 0 || packed.mode == 2);
                const u32 m1 = three ? (s_pm3[p] & 0xffffu) : (u32)s_pm2[p];
                const u32 m2 = three ? (s_pm3[p] >> 16) : 0u;
                const u32 m0 = ~(m1 | m2) & 0xffffu;
                const int n0 = __popc(m0), n1 = __popc(m1);
                const u64 cat = ((u64)packed.idxHi << 32) | packed.idxLo;
                u64 pos = 0;
#pragma unroll
                for (int t = 0; t < 4; t++)
                {
                    const int px = 4 * c + t;
                    const u32 below = (1u << px) - 1u;
                    const bool in1 = (m1 >> px) & 1u, in2 = (m2 >> px) & 1u;
                    const int k = in2 ? n0 + n1 + __popc(m2 & below) : in1 ? n0 + __popc(m1 & below) : __popc(m0 & below);
                    pos |= ((cat >> (4 * k)) & 0xfull) << (4 * px);
                }
                u32 lo = (u32)pos, hi = (u32)(pos >> 32);
                lo |= xorLane(lo, 1);
                hi |= xorLane(hi, 1);
                lo |= xorLane(lo, 2);
                hi |= xorLane(hi, 2);
                packed.idxLo = lo;
                packed.idxHi = hi;
            }
        }
        const int mode = packed.mode;
        u32 w0, w1, w2, w3;
        if (mode == 4 || mode == 5)
        {
            packed.idx2Lo = s_parked[lane >> 2][0];
            packed.idx2Hi = s_parked[lane >> 2][1];
        }
        if (mode == 4)
            packDualPlane<4>(packed, w0, w1, w2, w3);
        else if (mode == 5)
            packDualPlane<5>(packed, w0, w1, w2, w3);
        else
        {
        // mode description bit-fields (BC7 format)
        const int numSubsetsTab[8] = {3, 2, 3, 2, 1, 1, 1, 2};
        const int partitionBitsTab[8] = {4, 6, 6, 6, 0, 0, 0, 6};
        const int rgbBitsTab[8] = {4, 6, 5, 7, 5, 7, 7, 5};
        const int alphaBitsTab[8] = {0, 0, 0, 0, 6, 8, 7, 5};
        const int indexBitsTab[8] = {3, 3, 2, 2, 2, 2, 4, 2};
        const int alphaIndexBitsTab[8] = {0, 0, 0, 0, 3, 2, 0, 0};
        const int pBitModeTab[8] = {0, 1, 2, 0, 2, 2, 0, 0}; // 0 per endpoint, 1 per subset, 2 none
        int numSubsets = 0, partitionBits = 0, rgbBits = 0, alphaBits = 0, indexBits = 0, alphaIndexBits = 0, pBitMode = 0;
#pragma unroll
        for (int m = 0; m < 8; m++)
            if (mode == m)
            {
                numSubsets = numSubsetsTab[m];
                partitionBits = partitionBitsTab[m];
                rgbBits = rgbBitsTab[m];
                alphaBits = alphaBitsTab[m];
                indexBits = indexBitsTab[m];
                alphaIndexBits = alphaIndexBitsTab[m];
                pBitMode = pBitModeTab[m];
            }
        constexpr bool separateAlpha = false; // modes 4 and 5 have gone to packDualPlane; their branches below fold away
        const bool combinedAlpha = (mode == 6 || mode == 7);
        const int partition = packed.partOrIS;
        const int indexSelector = packed.partOrIS;

        u64 idx = ((u64)packed.idxHi << 32) | packed.idxLo;
        u64 idx2 = ((u64)packed.idx2Hi << 32) | packed.idx2Lo;
        u32 ep[3][2];
#pragma unroll
        for (int s = 0; s < 3; s++)
        {
            ep[s][0] = packed.ep[s][0];
            ep[s][1] = packed.ep[s][1];
        }
        const u64 ones = 0x1111111111111111ull;
        int fix1 = 0, fix2 = 0;

        if (separateAlpha)
        {
            bool flipRGB = ((idx >> (indexBits - 1)) & 1ull) != 0;
            bool flipAlpha = ((idx2 >> (alphaIndexBits - 1)) & 1ull) != 0;
            if (flipRGB)
                idx = ones * (u64)((1 << indexBits) - 1) - idx;
            if (flipAlpha)
                idx2 = ones * (u64)((1 << alphaIndexBits) - 1) - idx2;
            if (indexSelector)
            {
                const bool t = flipRGB;
                flipRGB = flipAlpha;
                flipAlpha = t;
            }
            if (flipRGB)
            {
                const u32 a = ep[0][0], b = ep[0][1];
                ep[0][0] = (a & 0xff000000u) | (b & 0x00ffffffu);
                ep[0][1] = (b & 0xff000000u) | (a & 0x00ffffffu);
            }
            if (flipAlpha)
            {
                const u32 a = ep[0][0], b = ep[0][1];
                ep[0][0] = (a & 0x00ffffffu) | (b & 0xff000000u);
                ep[0][1] = (b & 0x00ffffffu) | (a & 0xff000000u);
            }
        }
        else
        {
            u32 subsetMap = 0; // 2 bits per pixel
            if (numSubsets == 2)
            {
                fix1 = T->anchor2[partition & 63];
                const u32 bits = T->partition2[partition & 63];
#pragma unroll
                for (int px = 0; px < 16; px++)
                    subsetMap |= ((bits >> px) & 1u) << (2 * px);
            }
            else if (numSubsets == 3)
            {
                fix1 = T->anchor3[partition & 63][0];
                fix2 = T->anchor3[partition & 63][1];
                subsetMap = T->partition3[partition & 63];
            }
            const int hiBit = indexBits - 1;
            bool flip[3];
            flip[0] = ((idx >> hiBit) & 1ull) != 0;
            flip[1] = (numSubsets >= 2) && (((idx >> (4 * fix1 + hiBit)) & 1ull) != 0);
            flip[2] = (numSubsets >= 3) && (((idx >> (4 * fix2 + hiBit)) & 1ull) != 0);
            u64 flipMask = 0;
#pragma unroll
            for (int px = 0; px < 16; px++)
            {
                const int s = (subsetMap >> (2 * px)) & 3;
                const bool f = (s == 0) ? flip[0] : ((s == 1) ? flip[1] : flip[2]);
                if (f)
                    flipMask |= 0xfull << (4 * px);
            }
            const u64 inverted = ones * (u64)((1 << indexBits) - 1) - idx;
            idx = (idx & ~flipMask) | (inverted & flipMask);
            const u32 chMask = combinedAlpha ? 0xffffffffu : 0x00ffffffu;
#pragma unroll
            for (int s = 0; s < 3; s++)
                if (flip[s])
                {
                    const u32 a = ep[s][0], b = ep[s][1];
                    ep[s][0] = (a & ~chMask) | (b & chMask);
                    ep[s][1] = (b & ~chMask) | (a & chMask);
                }
        }

        // ---- bit packing: the (up to 66) fields of the block are dealt round-robin to the four
        // lanes of the quad, each lane shifts its fields to their absolute bit positions, and
        // the quad ORs the four partial blocks together ----
        u64 lo = 0, hi = 0;
        auto put = [&](u32 value, int off, int bits) {
            const u64 v = (u64)value;
            (void)bits;
            if (off < 64)
            {
                lo |= v << off;
                if (off > 56)
                    hi |= v >> (64 - off); // fields are at most 8 bits wide
            }
            else
                hi |= v << (off - 64);
        };
        // header
        int epBase = mode + 1;
        if (c == 0)
        {
            put(1u << mode, 0, mode + 1);
            if (partitionBits)
                put((u32)partition, epBase, partitionBits);
        }
        epBase += partitionBits;
        if (separateAlpha)
        {
            if (c == 1)
            {
                put((u32)packed.rotation, epBase, 2);
                if (mode == 4)
                    put((u32)indexSelector, epBase + 2, 1);
            }
            epBase += (mode == 4) ? 3 : 2;
        }
        // endpoints: channel-major, then subset, then endpoint 0/1; then alpha; then p-bits
        const int perChannel = 2 * numSubsets;
        const int numRGB = 3 * perChannel;
        const int numAlpha = alphaBits ? perChannel : 0;
        const int numPBits = (pBitMode == 0) ? perChannel : (pBitMode == 1) ? numSubsets : 0;
        const int alphaBase = epBase + numRGB * rgbBits;
        const int pBase = alphaBase + numAlpha * alphaBits;
        const int idxBase = pBase + numPBits;
        for (int i = 0; i < 8; i++)
        {
            const int f = 4 * i + c;
            if (__ballot(f < numRGB + numAlpha + numPBits) == 0)
                break;
            if (f < numRGB + numAlpha)
            {
                // colour or alpha endpoint field
                const bool isAlpha = f >= numRGB;
                const int g = isAlpha ? f - numRGB : f;
                const int ch = isAlpha ? 3 : ((numSubsets == 1) ? (g >> 1) : (numSubsets == 2) ? (g >> 2) : (g / 6));
                const int rem = isAlpha ? g : g - ch * perChannel;
                const int sub = rem >> 1, e = rem & 1;
                const u32 e0 = (sub == 0) ? ep[0][0] : (sub == 1) ? ep[1][0] : ep[2][0];
                const u32 e1 = (sub == 0) ? ep[0][1] : (sub == 1) ? ep[1][1] : ep[2][1];
                const u32 val = ((e ? e1 : e0) >> (8 * ch)) & 0xffu;
                const int bits = isAlpha ? alphaBits : rgbBits;
                put(val >> (8 - bits), isAlpha ? alphaBase + g * alphaBits : epBase + g * rgbBits, bits);
            }
            else if (f < numRGB + numAlpha + numPBits)
            {
                const int g = f - numRGB - numAlpha;
                const int sub = (pBitMode == 1) ? g : (g >> 1);
                const int e = (pBitMode == 1) ? 0 : (g & 1);
                const u32 e0 = (sub == 0) ? ep[0][0] : (sub == 1) ? ep[1][0] : ep[2][0];
                const u32 e1 = (sub == 0) ? ep[0][1] : (sub == 1) ? ep[1][1] : ep[2][1];
                put((((e ? e1 : e0) & 0xffu) >> (7 - rgbBits)) & 1u, pBase + g, 1);
            }
        }
        // indexes: pixel px at idxBase + px*indexBits minus one bit per anchor before it
#pragma unroll
        for (int i = 0; i < 4; i++)
        {
            const int px = 4 * i + c;
            const bool anchor = (px == 0 || px == fix1 || px == fix2);
            const int before = (px > 0 ? 1 : 0) + ((fix1 != 0 && px > fix1) ? 1 : 0) + ((fix2 != 0 && px > fix2) ? 1 : 0);
            put((u32)((idx >> (4 * px)) & 0xfull), idxBase + px * indexBits - before, indexBits - (anchor ? 1 : 0));
        }
        if (separateAlpha)
        {
            const int idx2Base = idxBase + 16 * indexBits - 1;
#pragma unroll
            for (int i = 0; i < 4; i++)
            {
                const int px = 4 * i + c;
                put((u32)((idx2 >> (4 * px)) & 0xfull), idx2Base + px * alphaIndexBits - (px > 0 ? 1 : 0), alphaIndexBits - (px == 0 ? 1 : 0));
            }
        }
        w0 = (u32)lo;
        w1 = (u32)(lo >> 32);
        w2 = (u32)hi;
        w3 = (u32)(hi >> 32);
#pragma unroll
        for (int step = 1; step <= 2; step <<= 1)
        {
            w0 |= xorLane(w0, step);
            w1 |= xorLane(w1, step);
            w2 |= xorLane(w2, step);
            w3 |= xorLane(w3, step);
        }
        }

        if (HARD)
        {
            if (valid && c == 0)
            {
                // nothing committed: no candidate from this slice
                const bool improved = (work.err != hardErr) || (workSeq != hardSeq);
                CvttBc7HardCand cand;
                cand.packed[0] = w0;
                cand.packed[1] = w1;
                cand.packed[2] = w2;
                cand.packed[3] = w3;
                cand.err = improved ? work.err : FLT_MAX;
                cand.seq = workSeq;
                BOUND_DUMP(bdEmit(BD_FINAL, BD_END, 0, 7, 2, 0, 0, 0, work.err, work.err, work.err, false, (float)workSeq));
                cand.pad[0] = cand.pad[1] = 0;
                A.hardCand[vBlock] = cand;
            }
        }
        else if (valid && c == 0)
        {
            uint4 o;
            o.x = w0;
            o.y = w1;
            o.z = w2;
            o.w = w3;
            *reinterpret_cast<uint4 *>(out + (size_t)blockIndex * 16u) = o;
            BOUND_DUMP(bdEmit(BD_FINAL, BD_END, 0, 0, 0, 0, 0, 0, work.err, work.err, work.err, false, (float)workSeq));
            if (!PT && A.hardCap != 0)
            {
                const u32 slot = s_blkFlags[blk] >> 8;
                if (slot != 0)
                {
                    CvttBc7HardRec &rec = A.hardRec[slot - 1u];
                    rec.blockIndex = blockIndex;
                    rec.err = work.err;
                    rec.seq = workSeq;
                }
            }
        }
    }
    PROF_MARK(5)
    PROF_TRACE
    PROF_FLUSH
}
#undef REFRESH_LANE
#undef valid
#undef anyBlockHasAlpha
#undef allowRGBModes
#undef allowMode7
#undef blockHasNonMaxAlpha
#undef WS_GET
#undef WS_SET

template <bool FAST, bool PT, bool HARD>
// (the punch-through instantiation holds 22 KB of LDS: two waves per SIMD is all that fits, so it may use their registers)
__global__ __launch_bounds__(64, PT ? 3 : (FAST || HARD) ? CVTT_BC7_WAVES : CVTT_BC7_WAVES_SLOW) void cvttmi_bc7_kernel(const uint8_t *__restrict__ blocks, uint8_t *__restrict__ out,
                                                        const CvttBc7Args A, const CvttDeviceTables *__restrict__ T,
                                                        const CvttBc7DevicePlan *__restrict__ dplan)
{
    if constexpr (!HARD)
    {
        // the counter of the NEXT encode's hand-over list (the two alternate, shim.cpp): nothing that read it is still running
        // (launches that use the list are ordered, orderAfterPrevious), and nothing of this encode touches it -- no memset launch
        if (!PT && A.hardCap != 0 && blockIdx.x == 0 && threadIdx.x == 0)
            *A.hardCountNext = 0u;
        bc7Body<FAST, PT, HARD>(blocks, out, A, T, dplan, blockIdx.x, gridDim.x);
    }
    else
    {
        // The second launch is a FIXED grid (cvttmi_launch_bc7: at most 4 096 waves) whose waves walk the items -- kHardWaves per
        // recorded block -- in strides of the grid.  On content that hands nothing over (RGBA noise) it used to be 16 waves per
        // SLOT, every one dispatched only to read the count and leave: 24 us of a 1.5 ms encode.
        const u32 count = *A.hardCount;
        const u32 total = (count < A.hardCap ? count : A.hardCap) * (u32)kHardWaves;
        for (u32 item = blockIdx.x; item < total; item += gridDim.x)
        {
            bc7Body<FAST, PT, HARD>(blocks, out, A, T, dplan, item, total);
            __syncthreads(); // the next item reuses the LDS of this one
        }
    }
}

// Third launch: the winner among the recorded best of a handed-over block and the candidates of its partition slices.
__global__ __launch_bounds__(64) void cvttmi_bc7_hard_commit_kernel(uint8_t *__restrict__ out, const CvttBc7Args A)
{
    const u32 h = blockIdx.x * 64u + threadIdx.x;
    const u32 count = *A.hardCount;
    if (h >= (count < A.hardCap ? count : A.hardCap))
        return;
    const CvttBc7HardRec rec = A.hardRec[h];
    float bestErr = rec.err;
    int bestSeq = rec.seq, best = -1;
    for (int q = 0; q < kHardWaves; q++)
    {
        const CvttBc7HardCand &cand = A.hardCand[h * kHardWaves + q];
        const float e = cand.err;
        const int sq = cand.seq;
        if (e == FLT_MAX)
            continue; // nothing from this slice
        if (e < bestErr || (e == bestErr && sq < bestSeq))
        {
            bestErr = e;
            bestSeq = sq;
            best = q;
        }
    }
    if (best >= 0)
    {
        const CvttBc7HardCand &cand = A.hardCand[h * kHardWaves + best];
        *reinterpret_cast<uint4 *>(out + (size_t)rec.blockIndex * 16u) = make_uint4(cand.packed[0], cand.packed[1], cand.packed[2], cand.packed[3]);
    }
}

extern "C" hipError_t cvttmi_launch_bc7(const void *d_blocks, void *d_out, const CvttBc7Args *args,
                                        const CvttDeviceTables *d_tables, const CvttBc7DevicePlan *d_plan,
                                        hipStream_t stream)
{
    const uint32_t waves = (args->numBlocks + 15u) / 16u;
    if (waves == 0)
        return hipSuccess;
    const bool fast = (args->flags & CVTTMI_FLAG_BC7_FAST_INDEXING) != 0;
    const bool pt = (args->flags & CVTTMI_FLAG_BC7_RESPECT_PUNCHTHROUGH) != 0;
#define CVTT_LAUNCH(F, P, H, GRID) hipLaunchKernelGGL((cvttmi_bc7_kernel<F, P, H>), dim3(GRID), dim3(64), 0, stream, (const uint8_t *)d_blocks, (uint8_t *)d_out, *args, d_tables, d_plan)
    if (pt) // no hand-over: this kernel does not clear the next encode's counter, so the shim gives it no slots
    {
        if (fast) CVTT_LAUNCH(true, true, false, waves); else CVTT_LAUNCH(false, true, false, waves);
        return hipGetLastError();
    }
    if (fast) CVTT_LAUNCH(true, false, false, waves); else CVTT_LAUNCH(false, false, false, waves);
    if (args->hardCap != 0) // (the counter is zero: the previous encode's first launch cleared it, the context's creation the first two)
    {
        // a fixed grid that walks the items (kHardWaves per recorded block): one resident generation at most
        const uint32_t hardItems = args->hardCap * (uint32_t)kHardWaves;
        const uint32_t hardGrid = hardItems < 4096u ? hardItems : 4096u;
        if (fast) CVTT_LAUNCH(true, false, true, hardGrid); else CVTT_LAUNCH(false, false, true, hardGrid);
        hipLaunchKernelGGL(cvttmi_bc7_hard_commit_kernel, dim3((args->hardCap + 63u) / 64u), dim3(64), 0, stream, (uint8_t *)d_out, *args);
    }
#undef CVTT_LAUNCH
    return hipGetLastError();
}