// What the host files of the C ABI (shim*.cpp, and only they) share: the context, the skeleton every entry point runs in,
// and the few helpers more than one of them uses.  Functions that cross files live in cvtt_shim, which has hidden visibility:
// the library exports the C ABI and nothing of this.
#ifndef CVTTMI_SHIM_INTERNAL_H
#define CVTTMI_SHIM_INTERNAL_H

#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>

#include "cvtt_device.h"
#include "cvtt_launchers.h"
#include "hip_owned.h"
#include "texture_formats.h"

// Every field starts out in its final empty state; cvttmi_create assigns what it reads from its arguments or the environment and
// builds the rest, and a context that is deleted half-built frees what exists (hip_owned.h).
struct __attribute__((visibility("hidden"))) cvttmi_context
{
    int device = 0;
    CvttDeviceTables hostTables = {};
    cvtt_owned::DeviceBuffer dTables;
    const CvttDeviceTables *tables() const { return dTables.as<CvttDeviceTables>(); }
    // plan staging: a small ring of device plan slots so back-to-back launches with
    // different plans never race with an in-flight kernel
    static const int kPlanSlots = 8;
    cvtt_owned::DeviceBuffer dPlans;
    cvtt_owned::PinnedBuffer pinnedPlans; // the staged plans in pinned memory: sources of the asynchronous uploads
    cvttmi_bc7_plan lastPlan[kPlanSlots] = {};
    bool planValid[kPlanSlots] = {};
    // launches that read a slot since it was last written: one event per stream that launched one (a slot is rewritten
    // only when every one of them has finished; more than kPlanUsers distinct streams: the oldest entry is waited for)
    static const int kPlanUsers = 4;
    struct PlanUse
    {
        hipStream_t stream = NULL;
        cvtt_owned::Event ev; // created on first use
        bool valid = false;
    } planUse[kPlanSlots][kPlanUsers];
    cvtt_owned::Event evPlanUp[kPlanSlots]; // recorded after the slot's upload, on the stream that did it
    hipStream_t planUpStream[kPlanSlots] = {};
    int nextPlanSlot = 0;
    // host-pointer entry points: a pipeline of chunks, each slot with its own staging and stream, so that the uploads of
    // the next chunks and the downloads of the previous ones overlap the search of the current one, and the searches of
    // neighbouring chunks (small launches: a chunk is two or three waves per SIMD) fill the device together
    static const int kPipeSlots = 4;
    struct PipeSlot
    {
        cvtt_owned::PinnedBuffer pinnedIn, pinnedOut;
        cvtt_owned::DeviceBuffer dIn, dOut;
        cvtt_owned::Stream stream;
        cvtt_owned::Event done;
    } pipe[kPipeSlots];
    size_t pipeInBytes = 0, pipeOutBytes = 0; // what every slot's staging holds at least
    hipStream_t stream() const { return pipe[0].stream; } // the context's private stream
    // calls may arrive from several host threads and on several streams, but the work buffers below exist once:
    // `mu` serialises the host side of a call, `evLast` orders its launches after the previous call's
    std::recursive_mutex mu;
    cvtt_owned::Event evLast;
    hipStream_t lastStream = NULL;
    bool lastValid = false;
    cvtt_owned::DeviceBuffer dPtTrial; // BC7_RespectPunchThrough with more than 2 refine rounds (kMaxPTRefine of bc7_kernel.hip): the trial-error table of a launch's waves
    size_t ptTableBytes = (size_t)256 << 20; // cap of that table per launch (256 MB; CVTTMI_BC7_PT_TABLE_KB, read when the context is created)
    bool exhaustive = false; // search every candidate even when it provably cannot win
    // the measure's partials (one per workgroup of a launch, decode_kernel.hip), allocated by the first measure; shared
    // like the hand-over list: its calls are ordered after the previous call that used work buffers (orderAfterPrevious)
    cvtt_owned::DeviceBuffer dMeasureSlab;
    // cvttmi_measure_error (host buffers): device copies of one chunk of packed blocks, sources, per-block values and the
    // chunk's totals, allocated by the first such call and kept (they grow with the bytes per block of the format)
    cvtt_owned::DeviceBuffer dMeasureHost;
    // cvttmi_resize_image_device: the tables of a call are built in page-locked memory and copied to the caller's work space on
    // the call's stream.  A ring of slots, each grown by the first call that needs more: a slot is rewritten only after the copy
    // that last read it has finished (its event), so calls queued back to back never wait for each other's kernels.  A call
    // with the sizes and the filter of a slot's tables copies them again without rebuilding them.
    static const int kResizeSlots = 4;
    struct ResizeSlot
    {
        cvtt_owned::PinnedBuffer pinned;
        cvtt_owned::Event ev; // created on first use; recorded after the slot's latest copy, on `stream`
        hipStream_t stream = NULL;
        bool inFlight = false, valid = false;
        uint32_t srcW = 0, srcH = 0, dstW = 0, dstH = 0, filter = 0; // the tables it holds
    } resizeSlot[kResizeSlots];
    int nextResizeSlot = 0;
    // BC7: blocks with many live mode-7 partitions are finished by a second launch (bc7_kernel.hip, HARD).
    // One set of buffers per context: launches of one context are expected on one stream at a time.  Two counters
    // alternate, so that no memset launch is needed: an encode counts into one and its first kernel clears the other,
    // which the next encode counts into.  That holds only if every encode that gets slots clears the other counter; the
    // punch-through kernel does not, so a punch-through encode gets none.
    struct HandOver
    {
        static const uint32_t kSlots = 8192;
        cvtt_owned::DeviceBuffer dCount; // the two counters (in 256 B)
        cvtt_owned::DeviceBuffer dRec;   // CvttBc7HardRec x kSlots
        cvtt_owned::DeviceBuffer dCand;  // CvttBc7HardCand x kSlots x kHardWaves
        int min = 8;              // live partitions of a wave from which its blocks are handed over; 0 = never
        int div = 128;
        int capOverride = 0;      // > 0: slots per launch (experiments)
        uint32_t parity = 0;      // the counter the next encode counts into
        uint32_t lastCap = 0;     // slots of the most recent BC7 encode (0: it had no hand-over) ...
        uint32_t lastCounter = 0; // ... and the counter it counted into

        uint32_t *counter(uint32_t which) const { return dCount.as<uint32_t>() + which; }
        // the settings are read when the context is created.  (The one member function the library has always exported, by accident
        // of its inline linkage; the export is kept, so that the dynamic symbol table stays what tests/golden/exports.txt lists.)
        __attribute__((visibility("default"))) hipError_t create()
        {
            if (getenv("CVTTMI_BC7_HARD_MIN")) min = atoi(getenv("CVTTMI_BC7_HARD_MIN"));
            if (getenv("CVTTMI_BC7_HARD_DIV")) div = atoi(getenv("CVTTMI_BC7_HARD_DIV"));
            div = div < 1 ? 1 : div;
            if (getenv("CVTTMI_BC7_HARD_CAP")) capOverride = atoi(getenv("CVTTMI_BC7_HARD_CAP"));
            hipError_t e;
            if ((e = dCount.reserve(256)) != hipSuccess || (e = dRec.reserve(sizeof(CvttBc7HardRec) * kSlots)) != hipSuccess ||
                (e = dCand.reserve(sizeof(CvttBc7HardCand) * kSlots * kHardWaves)) != hipSuccess)
                return e;
            return hipMemset(dCount.get(), 0, 256); // both counters start at zero; from then on every encode clears the next one's
        }
        // The hand-over fields of an encode's arguments (args.flags and args.prune already set).  Slots for one block in a
        // thousand: with the second-tier bounds few blocks of ordinary content keep many partitions; the slots bound the
        // extra wavefronts where every block does, and the second launch is sized for all of them.  Below half a million
        // blocks the two extra launches (about 25 us) cost more than the tail they remove (measured: 1024^2 -5 %, 2048^2
        // -1 %, 4096^2 +1 %, near-opaque alpha noise +7 %).
        void arm(CvttBc7Args &args, size_t numBlocks)
        {
            uint32_t cap = numBlocks >= (1u << 19) ? static_cast<uint32_t>(numBlocks / 1024) : 0u;
            if (capOverride > 0)
                cap = static_cast<uint32_t>(capOverride);
            cap = cap > kSlots ? kSlots : cap;
            const bool pt = (args.flags & CVTTMI_FLAG_BC7_RESPECT_PUNCHTHROUGH) != 0;
            args.hardCap = (args.prune && min > 0 && !pt) ? cap : 0u;
            args.hardMin = static_cast<uint32_t>(min);
            args.hardDiv = static_cast<uint32_t>(div);
            args.hardCount = counter(parity);
            args.hardCountNext = counter(parity ^ 1u);
            args.hardRec = dRec.as<CvttBc7HardRec>();
            args.hardCand = dCand.as<CvttBc7HardCand>();
            lastCap = args.hardCap;
            lastCounter = parity;
        }
        // a launch of `args` has been queued: it clears the other counter, which the next launch counts into
        void launched(CvttBc7Args &args)
        {
            if (!args.hardCap)
                return;
            parity ^= 1u;
            args.hardCount = counter(parity);
            args.hardCountNext = counter(parity ^ 1u);
        }
        // a launch of `args` failed: once the launches queued before it have finished, the counters are cleared, so that
        // whichever launch of the sequence failed the next encode starts clean
        void failed(const CvttBc7Args &args, hipStream_t stream)
        {
            if (!args.hardCap)
                return;
            (void)hipStreamSynchronize(stream);
            (void)hipMemset(dCount.get(), 0, 256);
        }
        hipError_t stats(uint32_t *handedOver, uint32_t *slots) const
        {
            uint32_t v = 0;
            const hipError_t e = lastCap ? hipMemcpy(&v, counter(lastCounter), sizeof(v), hipMemcpyDeviceToHost) : hipSuccess;
            if (handedOver) *handedOver = v;
            if (slots) *slots = lastCap;
            return e;
        }
    } handOver;
    // timing
    bool timing = false;
    cvtt_owned::Event evStart, evStop;
    double totalMs = 0.0;
    uint64_t launches = 0;
    std::string lastError;
};

namespace cvtt_shim __attribute__((visibility("hidden")))
{
    // shim.cpp
    int fail(cvttmi_context *ctx, int code, const char *what, hipError_t e = hipSuccess);
    void orderAfterPrevious(cvttmi_context *ctx, hipStream_t stream);
    void markLaunch(cvttmi_context *ctx, hipStream_t stream);
    // `launch(state, dOut, dIn, n, stream)` queues the work of n blocks; see hostPipeline in shim.cpp
    typedef int (*PipelineLaunch)(void *state, void *dOut, const void *dIn, size_t n, hipStream_t stream);
    int hostPipeline(cvttmi_context *ctx, uint8_t *out, const uint8_t *in, size_t numBlocks, size_t inBpb, size_t outBpb, PipelineLaunch launch,
                     void *state, bool zeroCopyOk);
    // the encoder of `format` (a known id) on device pointers, as the encode entries queue it; does the format need a plan?
    int encodeBlocks(cvttmi_context *ctx, int format, const cvttmi_options *options, const cvttmi_bc7_plan *plan,
                     const cvttmi_options *allocOptions, void *dOut, const void *dIn, size_t numBlocks, hipStream_t stream);
    bool encoderTakesPlan(int format);

    // The alignment rule of device pointers (cvtt_mi355x.h, "Buffers"): one element of what the pointer points at (a block,
    // a texel, a per-block value, a field of the totals; always a power of two), or 16 bytes where the element is larger --
    // the widest access any kernel makes through a caller's pointer.
    inline bool alignedTo(const void *p, size_t elementBytes)
    {
        const size_t a = elementBytes < 16 ? elementBytes : 16;
        return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
    }
    const char *const kMisaligned = "misaligned device pointer (cvtt_mi355x.h, Buffers: one block, or 16 bytes if smaller)";

    // the most blocks of one launch: its count is a uint32_t of the kernel arguments, with room to round up to whole waves
    const size_t kMaxLaunchBlocks = 0xfffffff0u;
    const uint32_t kMaxMipLevels = 32; // cvttmi_mip_level_count of the largest uint32_t sizes

    // every format (CVTTMI_FMT_*): its row of texture_formats.h, NULL for an unknown id; and, where asked for, bytes per
    // packed block, per decoded / source block, and the channels it stores
    inline const CvttTextureFormat *formatInfo(int format, size_t *bcBytes = NULL, size_t *texBytes = NULL, uint32_t *mask = NULL)
    {
        if (format < 0 || format >= CVTTMI_FMT_COUNT)
            return NULL;
        const CvttTextureFormat *row = &kCvttTextureFormats[format];
        if (bcBytes) *bcBytes = row->bcBytes;
        if (texBytes) *texBytes = row->texBytes;
        if (mask) *mask = row->mask;
        return row;
    }

    // `f` on the context's device, under its lock: calls may arrive from several host threads, and the error text, the
    // timing state and the work buffers exist once per context
    template <class F>
    int withDevice(cvttmi_context *ctx, F f)
    {
        const hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess)
            return fail(ctx, CVTTMI_E_NO_DEVICE, "hipSetDevice", e);
        std::lock_guard<std::recursive_mutex> lock(ctx->mu);
        return f();
    }

    // cvttmi_timing_enable: the device time between two events around `body` on its stream is added up
    template <class Body>
    int timed(cvttmi_context *ctx, hipStream_t stream, Body body)
    {
        if (!ctx->timing)
            return body();
        hipEventRecord(ctx->evStart, stream);
        const int rc = body();
        if (rc != CVTTMI_OK)
            return rc;
        hipEventRecord(ctx->evStop, stream);
        hipEventSynchronize(ctx->evStop);
        float ms = 0.0f;
        hipEventElapsedTime(&ms, ctx->evStart, ctx->evStop);
        ctx->totalMs += ms;
        ctx->launches += 1;
        return CVTTMI_OK;
    }

    // Every encode / decode entry point on device pointers: the common checks (argsOk: the entry's own checks of its other
    // arguments; inBpb / outBpb: bytes per block, for the alignment rule), then `body(dOut, dIn, numBlocks, stream)`, which
    // fills the format's arguments and queues its launches.
    template <class Body>
    int onDevice(cvttmi_context *ctx, void *dOut, const void *dIn, size_t numBlocks, bool argsOk, size_t inBpb, size_t outBpb,
                 void *hipStream, Body body)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        if (!dOut || !dIn || !argsOk || (numBlocks % 8) != 0 || numBlocks > kMaxLaunchBlocks)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (!alignedTo(dIn, inBpb) || !alignedTo(dOut, outBpb))
            return fail(ctx, CVTTMI_E_INVALID, kMisaligned);
        if (numBlocks == 0)
            return CVTTMI_OK;
        hipStream_t stream = static_cast<hipStream_t>(hipStream);
        return withDevice(ctx, [&] { return timed(ctx, stream, [&] { return body(dOut, dIn, numBlocks, stream); }); });
    }

    // ... and on host pointers: the same checks without the cap on the batch, then the same body for every launch of
    // hostPipeline (`inBpb` / `outBpb` bytes per block), each timed on its own
    template <class Body>
    int onHost(cvttmi_context *ctx, void *out, const void *in, size_t numBlocks, bool argsOk, size_t inBpb, size_t outBpb,
               bool zeroCopyOk, Body body)
    {
        if (!ctx)
            return CVTTMI_E_INVALID;
        if (!out || !in || !argsOk || (numBlocks % 8) != 0)
            return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
        if (numBlocks == 0)
            return CVTTMI_OK;
        auto launch = [&](void *dOut, const void *dIn, size_t n, hipStream_t stream) -> int {
            if (n > kMaxLaunchBlocks) // (the zero-copy paths hand the whole batch to one launch)
                return fail(ctx, CVTTMI_E_INVALID, "invalid argument");
            return timed(ctx, stream, [&] { return body(dOut, dIn, n, stream); });
        };
        typedef decltype(launch) Launch;
        const PipelineLaunch call = [](void *state, void *dOut, const void *dIn, size_t n, hipStream_t stream) -> int {
            return (*static_cast<Launch *>(state))(dOut, dIn, n, stream);
        };
        return withDevice(ctx, [&] {
            return hostPipeline(ctx, static_cast<uint8_t *>(out), static_cast<const uint8_t *>(in), numBlocks, inBpb, outBpb, call, &launch, zeroCopyOk);
        });
    }
}

#endif
