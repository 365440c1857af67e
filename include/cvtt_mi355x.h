/* cvtt_mi355x.h -- C ABI of the MI355X-native block-texture encoder.
 *
 * This is the drop-in boundary for the hot path of elasota/ConvectionKernels: the
 * per-block endpoint / partition / index search behind
 *     cvtt::Kernels::EncodeBC7        (reference ConvectionKernels.h:251, ConvectionKernels_API.cpp:41-54)
 *     cvtt::Kernels::EncodeBC1        (reference ConvectionKernels.h:242, ConvectionKernels_API.cpp:86-99)
 *     cvtt::Kernels::EncodeBC6HU/S    (reference ConvectionKernels.h:249-250, API.cpp:56-84)
 *     cvtt::Kernels::EncodeETC2[RGBA] (reference ConvectionKernels.h:253-254, API.cpp:216-229, 270-286)
 *
 * Plain pointers and sizes only.  The PODs below are byte-compatible with the reference's
 * cvtt::Options (ConvectionKernels.h:73-103, 44 bytes) and cvtt::BC7EncodingPlan
 * (ConvectionKernels.h:142-199, 808 bytes), so a reference user passes the address of the
 * structs they already have.
 *
 * Batch semantics: every encode call takes numBlocks (a multiple of 8) PixelBlocks stored
 * contiguously; group g = blocks [8g, 8g+8) is exactly what ONE call of the corresponding
 * cvtt::Kernels::Encode* consumes (ConvectionKernels.h:241), including the reference's
 * cross-lane coupling inside a group.  Output block i is bit-identical
 * to what the reference's SSE2 path writes for input block i.
 *
 * Error behaviour: the reference's entry points are void and assert on NULL
 * (ConvectionKernels_API.cpp:43-44).  Here every call returns 0 on success or a negative
 * CVTTMI_E_* code; nothing is written to the output on failure.  There is NO CPU fallback:
 * if no HIP device / kernel image is available the call fails with CVTTMI_E_NO_DEVICE.
 */
#ifndef CVTT_MI355X_H
#define CVTT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVTTMI_OK 0
#define CVTTMI_E_INVALID (-1)     /* NULL pointer, numBlocks not a multiple of 8, ... */
#define CVTTMI_E_UNSUPPORTED (-2) /* flag / format combination not implemented on the GPU path */
#define CVTTMI_E_NO_DEVICE (-3)   /* no HIP device, or device is not gfx950 */
#define CVTTMI_E_HIP (-4)         /* a HIP runtime call failed; see cvttmi_last_error() */

/* mirrors cvtt::Flags (ConvectionKernels.h:33-69) */
#define CVTTMI_FLAG_BC7_FAST_INDEXING 0x008u
#define CVTTMI_FLAG_BC7_TRY_SINGLE_COLOR 0x010u
#define CVTTMI_FLAG_BC7_RESPECT_PUNCHTHROUGH 0x020u
#define CVTTMI_FLAG_BC6H_FAST_INDEXING 0x040u
#define CVTTMI_FLAG_S3TC_EXHAUSTIVE 0x080u
#define CVTTMI_FLAG_S3TC_PARANOID 0x100u
#define CVTTMI_FLAG_UNIFORM 0x200u
#define CVTTMI_FLAG_ETC_USE_FAKE_BT709 0x400u
#define CVTTMI_FLAG_ETC_FAKE_BT709_ACCURATE 0x800u
#define CVTTMI_FLAGS_DEFAULT (CVTTMI_FLAG_BC7_FAST_INDEXING | CVTTMI_FLAG_S3TC_PARANOID)

/* byte image of cvtt::Options, ConvectionKernels.h:73-103 */
typedef struct cvttmi_options
{
    uint32_t flags;
    float threshold;
    float redWeight;
    float greenWeight;
    float blueWeight;
    float alphaWeight;
    int32_t refineRoundsBC7;
    int32_t refineRoundsBC6H;
    int32_t refineRoundsIIC;
    int32_t refineRoundsS3TC;
    int32_t seedPoints;
} cvttmi_options;

/* byte image of cvtt::BC7EncodingPlan, ConvectionKernels.h:142-199 */
typedef struct cvttmi_bc7_plan
{
    uint64_t mode1PartitionEnabled;
    uint64_t mode2PartitionEnabled;
    uint64_t mode3PartitionEnabled;
    uint16_t mode0PartitionEnabled;
    uint64_t mode7RGBAPartitionEnabled;
    uint64_t mode7RGBPartitionEnabled;
    uint8_t mode4SP[4][2];
    uint8_t mode5SP[4];
    uint8_t mode6Enabled;
    uint8_t seedPointsForShapeRGB[243];
    uint8_t seedPointsForShapeRGBA[129];
    uint8_t rgbaShapeList[129];
    uint8_t rgbaNumShapesToEvaluate;
    uint8_t rgbShapeList[243];
    uint8_t rgbNumShapesToEvaluate;
} cvttmi_bc7_plan;

/* byte image of cvtt::BC7FineTuningParams, ConvectionKernels.h:105-140: seed points (0 = off) per mode and
 * partition / rotation / index selector */
typedef struct cvttmi_bc7_fine_tuning
{
    uint8_t mode0SP[16];
    uint8_t mode1SP[64];
    uint8_t mode2SP[64];
    uint8_t mode3SP[64];
    uint8_t mode4SP[4][2];
    uint8_t mode5SP[4];
    uint8_t mode6SP;
    uint8_t mode7SP[64];
} cvttmi_bc7_fine_tuning;

typedef struct cvttmi_context cvttmi_context;

/* Default-constructed PODs (cvtt::Options(), cvtt::BC7EncodingPlan()). */
/* Build identity of this library: SHA-256 (hex) over its kernel / shim sources, public headers and compiler flags.  Not part
 * of the reference's API: measurement tooling uses it to tie rocprofv3 summaries to the library they were taken with. */
const char *cvttmi_source_sha256(void);

void cvttmi_default_options(cvttmi_options *out);
void cvttmi_default_bc7_plan(cvttmi_bc7_plan *out);
void cvttmi_default_bc7_fine_tuning(cvttmi_bc7_fine_tuning *out);

/* replace cvtt::Kernels::ConfigureBC7EncodingPlanFromQuality (ConvectionKernels_BC67.cpp:3291-3352; quality is
 * clamped to 1..100) and ConfigureBC7EncodingPlanFromFineTuningParams (BC67.cpp:3355-3483).  Host-side, once per job;
 * need no device.  The quality ladder is the reference's empirical ranking, carried as the observed plan changes per
 * quality step (csrc/bc7_quality_events.h, tools/gen_bc7_quality_events.py); plans are byte-identical to the reference's. */
int cvttmi_bc7_plan_from_quality(cvttmi_bc7_plan *plan, int quality);
int cvttmi_bc7_plan_from_fine_tuning(cvttmi_bc7_plan *plan, const cvttmi_bc7_fine_tuning *params);

/* Create a context on HIP device `device`: uploads the constant tables to HBM and
 * probes the host's RCPPS table (the reference's EndpointRefiner uses _mm_rcp_ps,
 * ConvectionKernels_EndpointRefiner.h:106, whose result is CPU-model specific; the
 * argument is always an integer 1..16, so the kernels take it as a 17-entry table and
 * "bit-exact vs. the CPU path on the same box" is well defined). */
int cvttmi_create(cvttmi_context **out, int device);
void cvttmi_destroy(cvttmi_context *ctx);
const char *cvttmi_last_error(const cvttmi_context *ctx);

/* Override / read the reciprocal table: lut[i] = rcpps(i), i = 1..16 (lut[0] ignored). */
int cvttmi_set_rcp_table(cvttmi_context *ctx, const float lut[17]);
int cvttmi_get_rcp_table(const cvttmi_context *ctx, float lut[17]);

/* Page-locked host memory.  The host-pointer entry points below (the ones the reference's own callers bind,
 * ConvectionKernels.h:242-256 take host pointers) move caller buffers that are page-locked straight over PCIe, in
 * chunks pipelined with the search; pageable buffers go through the context's staging buffers first (one extra CPU
 * copy each way).  cvttmi_host_alloc / cvttmi_host_free give such memory; cvttmi_host_register / _unregister
 * page-lock an existing allocation for as long as it is reused (registering costs about as much as one copy). */
int cvttmi_host_alloc(cvttmi_context *ctx, void **ptr, size_t bytes);
int cvttmi_host_free(cvttmi_context *ctx, void *ptr);
int cvttmi_host_register(cvttmi_context *ctx, void *ptr, size_t bytes);
int cvttmi_host_unregister(cvttmi_context *ctx, void *ptr);

/* Texture formats: the one id a format has from here to the kernel launchers -- the generic encode, decode, measure and
 * multi-device entries all take it.  cvttmi_format_info: bytes per packed block, bytes per input / decoded block (PixelBlockU8
 * 64, PixelBlockF16 128, PixelBlockScalarS16 32) and the channels the format stores (bit c = channel c), from the library's
 * one table; needs no context; CVTTMI_E_INVALID for an unknown id; any out pointer may be NULL. */
#define CVTTMI_FMT_BC7 0
#define CVTTMI_FMT_BC1 1
#define CVTTMI_FMT_BC6HU 2
#define CVTTMI_FMT_BC6HS 3
#define CVTTMI_FMT_ETC2_RGB 4
#define CVTTMI_FMT_ETC2_RGBA 5
#define CVTTMI_FMT_BC2 6
#define CVTTMI_FMT_BC3 7
#define CVTTMI_FMT_BC4U 8
#define CVTTMI_FMT_BC4S 9
#define CVTTMI_FMT_BC5U 10
#define CVTTMI_FMT_BC5S 11
#define CVTTMI_FMT_ETC1 12
#define CVTTMI_FMT_ETC2_PUNCHTHROUGH 13
#define CVTTMI_FMT_EAC_ALPHA 14
#define CVTTMI_FMT_R11U 15
#define CVTTMI_FMT_R11S 16
#define CVTTMI_FMT_COUNT 17
int cvttmi_format_info(int format, size_t *packedBytes, size_t *blockBytes, uint32_t *channelMask);

/* ---- device-resident entry points: d_blocks / d_out are HBM pointers on the context's
 * device; the launch is asynchronous on `hipStream` (a hipStream_t, NULL = default).
 * Streams: a context owns ONE set of device work space (BC7 hand-over list, punch-through trial table and plan ring; up to 256 MB
 * for the trial table, see below).  The calls that use it (EncodeBC7 from half a million blocks or with BC7_RespectPunchThrough and
 * more than 2 refine rounds) are ordered by the library itself: such a call on another stream than the
 * previous one first makes its stream wait (hipStreamWaitEvent) for that call's launches; a plan slot is rewritten only
 * after every launch that read it, on whatever stream, has finished.  Calls that use no shared work space (BC1-BC5, ETC,
 * EAC, decode, tiling) are simply queued on the stream given.  A mutex serialises the host side of EVERY call on a
 * context, so any stream / thread mix is safe on one context; it is not concurrent: use one context per stream (or per
 * worker thread, the reference's caller model, etc2packer.cpp:215-281) to overlap independent jobs.  (EncodeBC6H keeps its
 * whole search state on the chip since round 4: no work buffer, no ordering between its calls.)
 *
 * Buffers.  Every pointer may point into the middle of a larger allocation (a mip level, a shard, blocks [a, b) of a batch): a
 * call reads its inputs only, and writes exactly numBlocks x bytesPerBlock bytes from d_out on (the tiling calls: the block
 * counts documented with them; the measure: numBlocks per-block values and the 80 bytes of the totals) -- never a byte before
 * or behind, whatever the launch rounds its grid up to.  Input and output must not overlap.
 * Alignment of DEVICE pointers: one element of what the pointer points at, or 16 bytes where the element is larger.  That is
 *   blocks in and out (PixelBlockU8 / S8 / F16 / ScalarS16, packed and decoded blocks): min(bytes per block, 16), i.e. 8 for
 *     the 8-byte formats (BC1, BC4, ETC1, ETC2 RGB / punch-through, EAC alpha, R11) and 16 for everything else;
 *   images: the texel size (4 bytes RGBA8, 8 bytes RGBA16F), rowPitchBytes a multiple of it;
 *   per-block error values: 4 bytes;  cvttmi_error_totals: 8 bytes.
 * These are the widest accesses the kernels make through a caller's pointer (16-byte loads of PixelBlocks and 16-byte packed
 * blocks, 8-byte stores of 8-byte blocks, one texel of an image, one uint32 / float, the 64-bit fields of the totals).  A
 * device pointer that breaks the rule is rejected with CVTTMI_E_INVALID before anything is queued; nothing is written.
 * HOST pointers (the entry points without _device) need no alignment at all, like the reference's byte arrays: pageable and
 * misaligned page-locked buffers are staged, block-aligned page-locked ones are transferred in place. ---- */

/* Every encoder by format id: the entry points named after the reference's calls, below, are this call with their id, and
 * describe what each format reads, writes and uses of `options`.  format = CVTTMI_FMT_*; an unknown id is CVTTMI_E_INVALID.
 * plan: required for BC7 (NULL: CVTTMI_E_INVALID, nothing is launched), ignored by every other format.  allocOptions: read only
 * by ETC2 RGB / RGBA / punch-through -- the Options AllocETC2Data was given, see cvttmi_encode_etc2_with_data; NULL = `options`
 * -- and ignored elsewhere.  cvttmi_encode is the host-buffer form (see "host-buffer convenience entry points"). */
int cvttmi_encode_device(cvttmi_context *ctx, int format, void *d_out, const void *d_blocks, size_t numBlocks,
                         const cvttmi_options *options, const cvttmi_bc7_plan *plan,
                         const cvttmi_options *allocOptions, void *hipStream);
int cvttmi_encode(cvttmi_context *ctx, int format, void *out, const void *blocks, size_t numBlocks,
                  const cvttmi_options *options, const cvttmi_bc7_plan *plan, const cvttmi_options *allocOptions);

/* replaces cvtt::Kernels::EncodeBC7 (ConvectionKernels_API.cpp:41-54): numBlocks * 64 B
 * of PixelBlockU8 in, numBlocks * 16 B out. */
int cvttmi_encode_bc7_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                             const cvttmi_options *options, const cvttmi_bc7_plan *plan, void *hipStream);

/* replaces cvtt::Kernels::EncodeBC1 (ConvectionKernels_API.cpp:86-99 ->
 * S3TCComputer::PackRGB with alphaTest = true, ConvectionKernels_S3TC.cpp:717-1052):
 * numBlocks * 64 B of PixelBlockU8 in, numBlocks * 8 B out.  Uses options->threshold,
 * seedPoints, refineRoundsS3TC, the S3TC_Paranoid / Uniform flags and the channel weights. */
int cvttmi_encode_bc1_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                             const cvttmi_options *options, void *hipStream);

/* replaces cvtt::Kernels::EncodeBC6HU (isSigned = 0) / EncodeBC6HS (isSigned != 0)
 * (ConvectionKernels_API.cpp:56-84 -> BC6HComputer::Pack, ConvectionKernels_BC67.cpp:2665-3051):
 * numBlocks * 128 B of PixelBlockF16 (half bits as int16, RGBA, alpha ignored) in,
 * numBlocks * 16 B out.  Uses options->seedPoints, refineRoundsBC6H, the BC6H_FastIndexing /
 * Uniform flags and the channel weights.  Group g = blocks [8g, 8g+8) keeps the reference's
 * cross-lane coupling (duplicate-round skip, mode commit loop). */
int cvttmi_encode_bc6h_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                              const cvttmi_options *options, int isSigned, void *hipStream);

/* replace cvtt::Kernels::EncodeETC2 / EncodeETC2RGBA / EncodeETC2Alpha
 * (ConvectionKernels_API.cpp:216-229, 270-286, 246-256 -> ETCComputer::CompressETC2Block with
 * punchthroughAlpha = false, ConvectionKernels_ETC.cpp:1664-1887, and CompressETC2AlphaBlock,
 * 1889-2085).  numBlocks * 64 B of PixelBlockU8 in; 8 B (RGB, alpha) or 16 B (RGBA: EAC alpha
 * block then colour block) per block out.  The reference's ETC2CompressionData scratch
 * (AllocETC2Data / ReleaseETC2Data) has no counterpart: the kernels keep their scratch in
 * LDS.  These calls derive the two chroma axes of the sector split from options->{red,green,blue}Weight,
 * i.e. they behave like a caller who allocates with the options it encodes with; a caller whose two
 * Options differ uses cvttmi_encode_etc2_with_data[_device] below.
 * Uses the colour weights and the Uniform / ETC_UseFakeBT709 / ETC_FakeBT709Accurate flags. */
int cvttmi_encode_etc2_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                              const cvttmi_options *options, void *hipStream);
int cvttmi_encode_etc2_rgba_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                                   const cvttmi_options *options, void *hipStream);
int cvttmi_encode_etc2_alpha_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                                    const cvttmi_options *options, void *hipStream);

/* replaces cvtt::Kernels::EncodeETC1 (ConvectionKernels_API.cpp:201-214 -> ETCComputer::CompressETC1Block,
 * ConvectionKernels_ETC.cpp:2116-2126, CompressETC1BlockInternal 2624-2882 with both the individual and the
 * differential mode): numBlocks * 64 B of PixelBlockU8 in, 8 B per block out.  The ETC1CompressionData scratch
 * (AllocETC1Data / ReleaseETC1Data) has no counterpart.  Same flags as ETC2. */
int cvttmi_encode_etc1_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                              const cvttmi_options *options, void *hipStream);
int cvttmi_encode_etc1(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                       const cvttmi_options *options);

/* replaces cvtt::Kernels::EncodeETC2PunchthroughAlpha (ConvectionKernels_API.cpp:231-244 -> CompressETC2Block with
 * punchthroughAlpha = true, ConvectionKernels_ETC.cpp:1664-1887; EncodeVirtualTModePunchthrough 887-1264;
 * CompressETC1PunchthroughBlockInternal 2885-3082): GL_COMPRESSED_RGB8_PUNCHTHROUGH_ALPHA1_ETC2 blocks, 8 B each.
 * A pixel is transparent when alpha < floor(clamp(options->threshold, 0, 1) * 255 + 1).  Group g = blocks [8g, 8g+8)
 * keeps the reference's coupling: one transparent pixel anywhere in the group sends all eight blocks through the
 * punch-through modes as well, and the virtual-T candidate lists depend on the group's pixel counts. */
int cvttmi_encode_etc2_punchthrough_alpha_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                                                 const cvttmi_options *options, void *hipStream);
int cvttmi_encode_etc2_punchthrough_alpha(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                                          const cvttmi_options *options);

/* The reference fixes the two chroma axes when the scratch is ALLOCATED -- ETC2CompressionDataInternal's constructor
 * computes them from the Options given to AllocETC2Data (ConvectionKernels_ETC.cpp:3117-3145) -- while the error weights
 * come from the Options of each Encode call.  `allocOptions` = the Options the caller passed to AllocETC2Data (only its
 * red / green / blue weights are read; NULL = `options`).  kind: CVTTMI_ETC2_RGB = EncodeETC2, CVTTMI_ETC2_RGBA =
 * EncodeETC2RGBA, CVTTMI_ETC2_PUNCHTHROUGH = EncodeETC2PunchthroughAlpha (the three calls that take the scratch).  The three
 * values are aliases of what this entry has always taken, kept for its callers; it maps them to CVTTMI_FMT_ETC2_RGB / _RGBA /
 * _PUNCHTHROUGH and is cvttmi_encode[_device] with that id.  Any other kind is CVTTMI_E_INVALID. */
#define CVTTMI_ETC2_RGB 0
#define CVTTMI_ETC2_RGBA 1
#define CVTTMI_ETC2_PUNCHTHROUGH 4
int cvttmi_encode_etc2_with_data_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks,
                                        const cvttmi_options *options, const cvttmi_options *allocOptions, int kind, void *hipStream);
int cvttmi_encode_etc2_with_data(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                                 const cvttmi_options *options, const cvttmi_options *allocOptions, int kind);

/* ---- host-buffer convenience entry points: stage through pinned memory, launch, copy
 * back, synchronise.  Same semantics as the *_device calls. ---- */
int cvttmi_encode_bc7(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                      const cvttmi_options *options, const cvttmi_bc7_plan *plan);

int cvttmi_encode_bc1(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                      const cvttmi_options *options);

int cvttmi_encode_bc6h(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                       const cvttmi_options *options, int isSigned);

int cvttmi_encode_etc2(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                       const cvttmi_options *options);
int cvttmi_encode_etc2_rgba(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                            const cvttmi_options *options);
int cvttmi_encode_etc2_alpha(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                             const cvttmi_options *options);

/* Search strategy.  By default the kernels skip candidates (partitions / subsets) whose
 * rigorous error lower bound already exceeds the best candidate found so far -- an exact
 * branch-and-bound: the output is bit-identical to the exhaustive search the reference
 * performs.  exhaustive != 0 evaluates every candidate like the reference does (same output,
 * slower); the environment variable CVTTMI_EXHAUSTIVE=1 sets the default of new contexts. */
int cvttmi_set_exhaustive(cvttmi_context *ctx, int exhaustive);

/* ---- image -> PixelBlock tiling on the device (the caller side of the path: reference
 * etc2packer/etc2packer.cpp:215-247 cuts a linear image into groups of eight horizontally
 * adjacent 4x4 blocks, clamping reads at the right and bottom edges; 275-281 drops the blocks
 * that only pad the last group of a block row) ----
 * cvttmi_tiled_block_count: blocks the tiling produces = ceil(ceil(w/4)/8)*8 per block row
 *   (a multiple of 8, so every block row is made of whole groups) times ceil(h/4) rows.
 * cvttmi_tile_image_device: d_image = linear RGBA8 or RGBA16F image in HBM (rowPitchBytes
 *   between rows) -> d_blocks = PixelBlockU8 / PixelBlockF16 array of that many blocks.
 * cvttmi_compact_rows_device: packed blocks of the padded layout -> the ceil(w/4) real blocks of
 *   every row, contiguous (what a container writer stores).  A no-op copy when w % 32 == 0. */
#define CVTTMI_PIXELS_RGBA8 0
#define CVTTMI_PIXELS_RGBA16F 1
size_t cvttmi_tiled_block_count(uint32_t width, uint32_t height);
int cvttmi_tile_image_device(cvttmi_context *ctx, void *d_blocks, const void *d_image, uint32_t width, uint32_t height,
                             size_t rowPitchBytes, int pixelFormat, void *hipStream);
int cvttmi_compact_rows_device(cvttmi_context *ctx, void *d_out, const void *d_packed, uint32_t width, uint32_t height,
                               uint32_t bytesPerBlock, void *hipStream);

/* ---- mip chains (not part of the reference's API: its packer writes one level, etc2packer.cpp:116-197) ----
 * Level 0 is the image; level L+1 is max(1, w_L >> 1) x max(1, h_L >> 1); a full chain has floor(log2(max(w, h))) + 1 levels
 * and ends at 1x1.  cvttmi_mip_level_count gives that number (0 when a size is 0).
 * Filter: a 2x2 box over texels (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1) of level L, coordinates clamped to w_L - 1 and
 * h_L - 1 (that only matters when a dimension is already 1; an odd dimension drops its last column / row: the usual floor
 * convention).  Every level is computed from the ROUNDED level before it.  Per channel:
 *   CVTTMI_PIXELS_RGBA8        (a + b + c + d + 2) >> 2 on unsigned bytes
 *   CVTTMI_PIXELS_RGBA8_SNORM  the same on the bytes read as int8, in int32, arithmetic shift: floor((sum + 2) / 4) -- the
 *                              images BC4S / BC5S are encoded from.  Only the two mip calls take this constant.
 *   CVTTMI_PIXELS_RGBA16F      half -> float, ((a + b) + (c + d)) * 0.25f in that order, -> half round-to-nearest-even.  Finite
 *                              inputs are the contract: non-finite values propagate as IEEE arithmetic does, NaN bits unspecified.
 * That is CVTTMI_MIP_FILTER_BOX, the rule of cvttmi_build_mips_device.  cvttmi_build_mips_filtered_device takes a filter; the
 * geometry, the clamp, the rounded levels and the layout are the same for all of them, and channel 3 always takes the box rule of
 * its kind.  Channels 0..2, for the four texels a, b, c, d of a quad:
 *   CVTTMI_MIP_FILTER_SRGB (RGBA8)  averages in linear light.  Two tables from the sRGB EOTF lin(e) = e / 12.92 for e <= 0.04045,
 *       ((e + 0.055) / 1.055)^2.4 otherwise, computed in double precision (tools/gen_srgb_tables.py, cvttmi_srgb_tables):
 *         T[v] = floor(65535 lin(v / 255) + 0.5), v = 0..255;   U[k] = ceil(4 * 65535 lin((k - 0.5) / 255)), k = 1..255
 *       S = T[a] + T[b] + T[c] + T[d];  out = encode(S) = the number of k with S >= U[k].  Four equal texels give themselves.
 *   CVTTMI_MIP_FILTER_BOX | CVTTMI_MIP_FILTER_ALPHA_WEIGHTED (RGBA8)  A = sum of the four alphas, N = sum of value_i * alpha_i;
 *       A == 0: the box rule; otherwise out = (2 N + A) / (2 A), unsigned integer division (the weighted mean, rounded to nearest).
 *   CVTTMI_MIP_FILTER_SRGB | CVTTMI_MIP_FILTER_ALPHA_WEIGHTED (RGBA8)  N = sum of T[value_i] * alpha_i;  A == 0: S as for SRGB,
 *       otherwise S = (4 N + (A >> 1)) / A, unsigned integer division in 32 bits;  out = encode(S).
 *   CVTTMI_MIP_FILTER_NORMAL (RGBA8, RGBA8_SNORM)  renormalises.  Per texel and channel X = 2 v - 255 (RGBA8) or max(v, -127)
 *       (SNORM); SX, SY, SZ the integer sums over the four texels; Q = SX^2 + SY^2 + SZ^2 (below 2^24).  Q == 0: the box rule for
 *       all three channels.  Otherwise len = sqrtf((float)Q), q = (float)SX / len (IEEE single precision, correctly rounded), and
 *       RGBA8: out = clamp((int)floorf(q * 127.5f + 128.0f), 0, 255);  SNORM: out = clamp((int)floorf(q * 127.0f + 0.5f), -127, 127)
 *       -- the product and the sum are two separately rounded operations.
 * RGBA8 takes every filter above, RGBA8_SNORM takes BOX and NORMAL, RGBA16F takes BOX; NORMAL | ALPHA_WEIGHTED and every other
 * value are rejected (CVTTMI_E_INVALID with an error text, nothing written).  Otherwise the call is cvttmi_build_mips_device:
 * the same checks, one launch per level, exactly the levels' bytes written.
 * Mip kernels and wrap modes.  The `filter` word of the calls below has two more fields: a kernel in bits 4-7 (0: the 2x2 rules
 * above, untouched) and a wrap mode in bits 9-10.  Under a kernel the geometry, the rounded levels, the layout and the launch per
 * level stay; only the footprint of an output texel grows from 2x2 to n x n source texels, n = 4 R taps per direction:
 *   CVTTMI_MIP_KERNEL_TRIANGLE  R = 1  1 - |t|                     CVTTMI_MIP_KERNEL_LANCZOS3  R = 3  sinc(t) sinc(t / 3)
 *   CVTTMI_MIP_KERNEL_MITCHELL  R = 2  Mitchell-Netravali B = C = 1/3   CVTTMI_MIP_KERNEL_KAISER  R = 3  sinc(t) I0(4 sqrt(1 - (t/3)^2)) / I0(4)
 * Output column x is centred between source columns 2x and 2x + 1; tap k = 0 .. n - 1 reads source column 2x + 1 - 2R + k, wrapped
 * (rows alike), and sits t_k = (k - n/2 + 0.5) / 2 destination texels from the centre -- the same for every output texel, so a
 * kernel is ONE table w[0 .. n-1] (tools/gen_mip_kernels.py, cvttmi_mip_kernel_taps): the float64 weights divided by their sum,
 * each quantised as floor(16384 w + 0.5), what is missing to 16384 split equally between the two central taps:
 *   triangle  2048 6144 6144 2048                                                      sum |w| = 16384
 *   mitchell  -121 -192 2098 6407 6407 2098 -192 -121                                  sum |w| = 17636
 *   lanczos3  60 247 -557 -1092 2220 7314 7314 2220 -1092 -557 247 60                  sum |w| = 22980
 *   kaiser    103 266 -556 -1076 2195 7260 7260 2195 -1076 -556 266 103                sum |w| = 22912
 * An odd last column / row is no longer dropped (it is read as a neighbour); a dimension that is already 1 reproduces itself.
 * Wrap: 0 clamps a coordinate to the edge; CVTTMI_MIP_WRAP_REPEAT takes it modulo the size; CVTTMI_MIP_WRAP_MIRROR reflects with
 * the edge texel repeated once (-1 -> 0, w -> w - 1, period 2 w), correct however many times the footprint exceeds the image.
 * Arithmetic: two passes, horizontal then vertical, int32 throughout, arithmetic shifts; no intermediate is clamped.
 *   plain rule (CVTTMI_MIP_FILTER_BOX under a kernel; channel 3 always), v = the byte as uint8 / int8:
 *       h = sum w_k v_k;  h' = (h + 512) >> 10  (four fraction bits, |h'| <= 5723);  s = sum w_j h'_j;
 *       out = clamp((s + 2^17) >> 18, 0..255 or -128..127)
 *   CVTTMI_MIP_FILTER_SRGB, channels 0..2, v = T[byte]:  h' = (h + 2^13) >> 14;  s = sum w_j h'_j;
 *       S = clamp((s + 2^11) >> 12, 0, 4 * 65535);  out = encode(S) as above.  (|h| <= 1.51e9, |s| <= 1.6e9: below 2^31.)
 *   CVTTMI_MIP_FILTER_NORMAL, channels 0..2: the plain two passes on X (as above) up to s_c;  S_c = (s_c + 2^7) >> 8 (10 fraction bits,
 *       |S_c| < 2^20: exact as a float).  All three S_c zero: the plain rule on the three channels' bytes.  Otherwise, in IEEE single
 *       precision, every operation rounded on its own: len = sqrtf((fx * fx + fy * fy) + fz * fz), q = fS_c / len, and the two
 *       re-encode formulas above applied to q.
 * RGBA16F under a kernel.  A kernel with negative lobes rings below zero in HDR data (on a log-normal test image 28 % of the texels
 * of a Lanczos3 level are negative before any clamp), so the caller states the range of the results with one of two flags of the
 * filter word, CVTTMI_MIP_HDR_NONNEGATIVE: results clamped to [+0, 65504], or CVTTMI_MIP_HDR_SIGNED: to [-65504, 65504].  Valid
 * words: a flag goes only with CVTTMI_PIXELS_RGBA16F and the rule field CVTTMI_MIP_FILTER_BOX (the plain rule); in the mip calls
 * only together with a kernel (the 2x2 box of RGBA16F stays exactly what it is), in the resize calls with any kernel code, 0
 * included; exactly one of the two is required.  Geometry, taps, first taps, wraps and Q14 tables are those of the RGBA8 rules.
 * Arithmetic, per channel, all four channels alike, in IEEE binary32 round-to-nearest-even, every product and every sum rounded on
 * its own (no fused multiply-add):
 *       w_k = (float)q_k * 2^-14 (exact);  v = the half converted to float (exact)
 *       horizontal: h = +0.0f;  for k = 0 .. n-1 in index order: h = h + (w_k * v_k)
 *       vertical:   s = +0.0f;  for j in index order: s = s + (w_j * h_j)
 *       c = s < lo ? lo : (s > 65504.0f ? 65504.0f : s), lo = +0.0f (NONNEGATIVE) or -65504.0f (SIGNED);  out = half(c), round to
 *       nearest even, half subnormals produced, not flushed.
 *   No binary32 subnormal can arise (every intermediate is 0 or at least 2^-52 in magnitude); the sums never hold -0, because they
 *   start from +0; under SIGNED a small negative s converts to 0x8000, as IEEE conversion does; under NONNEGATIVE every s <= 0 gives
 *   0x0000.  Finite inputs are the contract, as for the box: with non-finite inputs only the texels whose footprint holds one are
 *   affected -- a NaN stays a NaN (bits unspecified), +-Inf sums are clamped like any value.  The restatement in numpy float32 is
 *   exact (tests/hdr_resample_ref.py); a fused step would not be, since emulating it through float64 rounds twice.
 * With a kernel RGBA8 takes BOX, SRGB and NORMAL, RGBA8_SNORM BOX and NORMAL, RGBA16F BOX with one range flag, under any one wrap
 * mode.  CVTTMI_E_INVALID with an error text, nothing queued, nothing written: a kernel with RGBA16F and no range flag, both range
 * flags, a range flag with RGBA8 / RGBA8_SNORM, with SRGB / NORMAL / ALPHA_WEIGHTED or without a kernel, a kernel with
 * ALPHA_WEIGHTED (the weighted mean's denominator can turn negative: what to do there is a decision of its own), a wrap flag without
 * a kernel, both wrap flags, an unknown kernel code, and any other bit (0x800 among them).
 * cvttmi_mip_kernel_taps: host only, no context.  Copies the table of the word's kernel to taps[0 .. 11] (zeros beyond *count = n);
 * CVTTMI_E_INVALID for kernel 0, an unknown kernel or a NULL pointer.
 * cvttmi_srgb_tables: host only, no context.  Copies T and U (U[k] at thresholds[k - 1]); CVTTMI_E_INVALID for a NULL pointer.
 * cvttmi_mip_layout: host only, no context.  Fills out[0 .. levels - 1] with each level's place in three buffers, and
 * out[levels] (so `out` has levels + 1 entries) with their ends = the three total sizes:
 *   the pyramid   levels 1 .. levels-1 as images with tightly pitched rows, each level starting on a 256-byte boundary of the
 *                 buffer (byteOffset, rowPitchBytes; both 0 for level 0, which stays where the caller has it);
 *                 out[levels].byteOffset = bytes the pyramid needs (0 for one level)
 *   the tiles     ONE PixelBlock buffer for all levels (firstTile, tileCount = cvttmi_tiled_block_count(w_L, h_L)): every
 *                 level is whole groups of eight, so one cvttmi_encode_device call covers the chain;
 *                 out[levels].firstTile = blocks of that buffer
 *   the output    the ceil(w_L/4) x ceil(h_L/4) packed blocks of each level, levels consecutive = container order
 *                 (firstBlock, blockCount, packedByteOffset = firstBlock x bytesPerBlock); out[levels].firstBlock = all blocks
 * CVTTMI_E_INVALID, nothing written: NULL out, a zero size, an unknown pixel kind, bytesPerBlock not 8 or 16, levels 0 or more
 * than cvttmi_mip_level_count, a pyramid beyond size_t.
 * cvttmi_build_mips_device: level 1 from d_image (rowPitchBytes between rows), every later level from the one before it in
 * d_pyramid; one launch per level on hipStream; levels == 1 launches nothing (d_pyramid may then be NULL).  Writes exactly the
 * levels' bytes: the gaps that align a level's start are not touched.  d_image / d_pyramid: aligned to the texel (4 / 8 bytes);
 * where the image's rows and the pyramid also start on 16-byte boundaries (any hipMalloc'ed pyramid) and a level's width is a
 * multiple of 16 bytes, the level is made with 16-byte accesses.  CVTTMI_E_INVALID before anything is queued: NULL pointers,
 * levels 0 or too many, pyramidBytes below out[levels].byteOffset, an unknown pixel kind, rowPitchBytes below the row or no
 * multiple of the texel, a misaligned pointer.  Image and pyramid must not overlap.
 * A chain is encoded by cvttmi_encode_texture_device (below, with layers = 1), or by hand: tile every level into its slot of the
 * tile buffer (cvttmi_tile_image_device takes a row pitch and any output offset), encode once, compact every level into its slot
 * of the output. */
#define CVTTMI_PIXELS_RGBA8_SNORM 2
typedef struct cvttmi_mip_level
{
    uint32_t width, height;
    size_t byteOffset, rowPitchBytes; /* in the pyramid */
    size_t firstTile, tileCount;      /* in the tiled PixelBlock buffer, in blocks */
    size_t firstBlock, blockCount;    /* in the packed output, in blocks */
    size_t packedByteOffset;          /* = firstBlock x bytesPerBlock */
} cvttmi_mip_level;
uint32_t cvttmi_mip_level_count(uint32_t width, uint32_t height);
int cvttmi_mip_layout(uint32_t width, uint32_t height, int pixelFormat, uint32_t bytesPerBlock, uint32_t levels, cvttmi_mip_level *out);
int cvttmi_build_mips_device(cvttmi_context *ctx, void *d_pyramid, size_t pyramidBytes, const void *d_image, uint32_t width,
                             uint32_t height, size_t rowPitchBytes, int pixelFormat, uint32_t levels, void *hipStream);
#define CVTTMI_MIP_FILTER_BOX 0
#define CVTTMI_MIP_FILTER_SRGB 1
#define CVTTMI_MIP_FILTER_NORMAL 2
#define CVTTMI_MIP_FILTER_ALPHA_WEIGHTED 0x100 /* a flag, OR-ed onto BOX or SRGB */
#define CVTTMI_MIP_KERNEL_TRIANGLE 0x10 /* bits 4-7: a kernel, OR-ed onto BOX, SRGB or NORMAL; 0 = the 2x2 rule */
#define CVTTMI_MIP_KERNEL_MITCHELL 0x20
#define CVTTMI_MIP_KERNEL_LANCZOS3 0x30
#define CVTTMI_MIP_KERNEL_KAISER 0x40
#define CVTTMI_MIP_WRAP_REPEAT 0x200 /* bits 9-10: how a kernel's taps leave the image; 0 = clamp to the edge */
#define CVTTMI_MIP_WRAP_MIRROR 0x400
#define CVTTMI_MIP_HDR_NONNEGATIVE 0x1000 /* RGBA16F under a kernel / in a resize: results clamped to [+0, 65504] */
#define CVTTMI_MIP_HDR_SIGNED 0x2000      /* ... clamped to [-65504, 65504]; exactly one of the two */
int cvttmi_build_mips_filtered_device(cvttmi_context *ctx, void *d_pyramid, size_t pyramidBytes, const void *d_image, uint32_t width,
                                      uint32_t height, size_t rowPitchBytes, int pixelFormat, uint32_t levels, uint32_t filter,
                                      void *hipStream);
int cvttmi_srgb_tables(uint16_t toLinear[256], uint32_t thresholds[255]);
int cvttmi_mip_kernel_taps(uint32_t filter, int16_t taps[12], uint32_t *count);

/* ---- resize: any source size to any destination size, up or down (not part of the reference's API) ----
 * The Q14 two-pass rule of the mip kernels above with one weight row per output column and one per output row, where the mip
 * kernels have one table for every texel.  The `filter` word is theirs: rule | kernel | wrap, rule = CVTTMI_MIP_FILTER_BOX (the
 * plain rule), _SRGB or _NORMAL, wrap = 0 (clamp) or one CVTTMI_MIP_WRAP_* flag.  Kernel: the four CVTTMI_MIP_KERNEL_* codes, R = 1,
 * 2, 3, 3, with the weight functions K(t) above, and -- in the resize calls only -- kernel code 0 = an area-average box (R = 1/2).
 * The rule of one axis, src texels resized to dst texels (both 1 .. 65535), big = max(src, dst); everything up to the weights is
 * integer arithmetic.  Going down the kernel is stretched by big / dst, going up it is not.
 *   taps per row    n = ceil(2R big / dst);  box: n = ceil(big / dst) + 1
 *   first tap       L = (2x + 1) src - dst - 2R big;  first[x] = floor(L / (2 dst)) + 1;  box: first[x] = floor((L + dst) / (2 dst)).
 *                   Tap k of output x reads source coordinate first[x] + k (may be negative or >= src), wrapped as above.
 *   weights         t = (double)(2 dst (first[x] + k) - (2x + 1) src + dst) / (double)(2 big);  w_k = K(t) in double precision;
 *                   W = the sum of the w_k, added in index order;  q_k = floor(16384 (w_k / W) + 0.5)
 *   box weights     exact integers in units of 1 / (2 dst): o_k = the overlap of [2 dst j - dst, 2 dst j + dst), j = first[x] + k, with
 *                   [(2x + 1) src - dst - big, (2x + 1) src - dst + big) (the overlaps sum to 2 big);
 *                   q_k = (2 * 16384 o_k + 2 big) / (4 big), integer division
 *   the row's sum   what is missing to 16384 goes to the taps that hold the row's largest q, divided equally among them (the
 *                   quotient truncated towards zero); the lowest index of them takes what does not divide.
 *   dst = src       every row is a single 16384 at the tap that reads x, the others 0: an image resized to its own size is itself.
 *                   The formulas above give exactly that for every kernel but Mitchell, whose K(0) = 8/9 would blur the image.
 * At dst = src / 2 the rows are the mip kernels' table and first[x] = 2x + 1 - 2R.
 * Guard: with P the largest sum of positive taps over the rows of a table, the table is refused (CVTTMI_E_INVALID) unless
 * 65535 P < 2^31 and ((65535 P + 8192) >> 14) (2P - 16384) < 2^31 -- the int32 sums of both passes under every rule (the largest
 * P observed is 20 870, Lanczos3).
 * Arithmetic: exactly that of the mip kernels -- horizontal then vertical, int32, arithmetic shifts, no intermediate clamp --
 * with the weight row of the output column in the first pass and of the output row in the second:
 *   plain rule, and always channel 3:  h' = (h + 512) >> 10;  out = clamp((s + 2^17) >> 18, 0..255 or -128..127)
 *   CVTTMI_MIP_FILTER_SRGB and _NORMAL: word for word as stated above for kernels.
 * RGBA8 takes the plain rule, SRGB and NORMAL; RGBA8_SNORM the plain rule and NORMAL; ALPHA_WEIGHTED is refused for the reason given
 * above for kernels.  RGBA16F takes the plain rule with exactly one CVTTMI_MIP_HDR_* flag, under any kernel code, the box (0)
 * included: the float arithmetic stated above under "RGBA16F under a kernel", word for word, with the weight row of the output column
 * in the first pass and of the output row in the second, the tables, first taps and wraps of this section.  Without a flag RGBA16F is
 * refused, and so are both flags, a flag with RGBA8 / RGBA8_SNORM and a flag with SRGB, NORMAL or ALPHA_WEIGHTED.  At exactly half
 * the size the result is the mip kernel's level; at the same size it is the image, but for what the range clamps, -0 (which becomes
 * +0) and NaN bits.
 * cvttmi_resize_taps: host only, no context; the one owner of the rule (the device call uses its output).  Reports *tapsPerRow = n;
 *   with weights != NULL it also fills weights[x * n + k] (dst x n values) and first[x] (dst values).  Only the kernel field of
 *   `filter` matters to the table; the word must be a valid one (of RGBA8, or of RGBA16F: the plain rule with one range flag).
 *   CVTTMI_E_INVALID: a size of 0 or above 65535, a word that is none, NULL tapsPerRow, weights without first, a table the guard refuses.
 * cvttmi_resize_work_bytes: host only, no context.  *workBytes = what cvttmi_resize_image_device needs at d_work for these
 *   arguments: the tables of both axes and, where the resize takes two launches, the intermediate (layers x srcH x dstW entries
 *   of 8 bytes, 16 under SRGB and NORMAL and for RGBA16F).  cvttmi_resize_launches: *launches = 1 where the source rows under every tile of 64 x 16
 *   output texels fit in LDS (52 KB), 2 otherwise.  Both reject (CVTTMI_E_INVALID) what the device call rejects
 *   of these arguments.
 * cvttmi_resize_image_device: `layers` images of srcW x srcH at d_src (srcRowPitchBytes between rows, srcLayerPitchBytes between
 *   layers) -> dstW x dstH at d_dst, everything on hipStream, the layer in the grid's z.  d_work: caller memory on a 256-byte
 *   boundary, at least workBytes = cvttmi_resize_work_bytes(..); its contents after the call are unspecified.  The tables are
 *   built in page-locked memory of the context (a ring of four slots, each grown by the first call that needs more; a call with
 *   the sizes and kernel of a slot's tables does not build them again) and copied to d_work on hipStream: calls queued back to
 *   back wait for nothing but, after four later tables, the copy that read a slot.  Nothing else is allocated.  Writes exactly dstW x 4
 *   (RGBA16F: dstW x 8) bytes of each of the dstH rows of each layer -- not the pitch gaps -- and nothing outside d_work[0, workBytes).
 *   Source and destination must not overlap.  CVTTMI_E_INVALID with an error text before anything is queued, nothing written: NULL
 *   pointers, d_src / d_dst not on a 4-byte (RGBA16F: 8-byte), d_work not on a 256-byte boundary, a size or layers of 0 or above 65535,
 *   a row pitch below the row or no multiple of 4 (8), a layer pitch below height x row pitch or no multiple of 4 (8), workBytes too
 *   small, an unknown pixel kind, RGBA16F without exactly one range flag, a range flag with anything but RGBA16F and the plain rule,
 *   SRGB with RGBA8_SNORM, ALPHA_WEIGHTED or any other rule, an unknown kernel code, both wrap flags, a refused table. */
int cvttmi_resize_taps(uint32_t src, uint32_t dst, uint32_t filter, int16_t *weights, int32_t *first, uint32_t *tapsPerRow);
int cvttmi_resize_work_bytes(uint32_t srcW, uint32_t srcH, uint32_t dstW, uint32_t dstH, int pixelFormat, uint32_t filter, uint32_t layers,
                             size_t *workBytes);
int cvttmi_resize_launches(uint32_t srcW, uint32_t srcH, uint32_t dstW, uint32_t dstH, int pixelFormat, uint32_t filter, uint32_t *launches);
int cvttmi_resize_image_device(cvttmi_context *ctx, void *d_dst, uint32_t dstW, uint32_t dstH, size_t dstRowPitchBytes, size_t dstLayerPitchBytes,
                               const void *d_src, uint32_t srcW, uint32_t srcH, size_t srcRowPitchBytes, size_t srcLayerPitchBytes,
                               int pixelFormat, uint32_t layers, uint32_t filter, void *d_work, size_t workBytes, void *hipStream);

/* ---- texture arrays and cube maps (not part of the reference's API) ----
 * A texture is `layers` images of one size, each with `levels` mip levels; layers = array elements x faces.  A cube is 6 layers
 * in the order +X -X +Y -Y +Z -Z, a cube array 6 n layers.  Every layer has the chain of cvttmi_mip_layout; with T = that
 * function's table for (width, height, pixelFormat, bytesPerBlock, levels) and E = T[levels].firstBlock, the packed output of
 * the whole texture holds layers x E blocks in one of two orders:
 *   CVTTMI_ORDER_LAYER_MAJOR  every layer's whole chain is consecutive (DDS):
 *                             (layer, level) starts at block  layer * E + T[level].firstBlock
 *   CVTTMI_ORDER_LEVEL_MAJOR  every level's layers are consecutive (KTX):
 *                             (layer, level) starts at block  layers * T[level].firstBlock + layer * T[level].blockCount
 * and holds T[level].blockCount blocks, row-major.  cvttmi_texture_subresource is the one owner of these two formulas.
 * cvttmi_texture_layout: host only, no context; built on cvttmi_mip_layout's table.  pyramidLayerBytes = T[levels].byteOffset
 *   rounded up to 256 (0 for one level), pyramidBytes = layers x that; tilesPerLayer = T[levels].firstTile, blocksPerLayer = E,
 *   tiles / blocks = layers x those; workBytes = what cvttmi_encode_texture_device needs at d_work.  (The struct is named
 *   cvttmi_texture_sizes: C has one name space for functions and typedefs.)
 *   CVTTMI_E_INVALID, nothing written: NULL out, layers == 0, an unknown order, 2^32 or more tiles or blocks in total, any size
 *   beyond size_t, and everything cvttmi_mip_layout rejects.
 * cvttmi_texture_subresource: the same arguments and checks, and layer < layers, level < levels; either result pointer may be NULL.
 * cvttmi_build_mips_array_device: cvttmi_build_mips_filtered_device for every layer.  Layer l's level 0 is at d_images +
 *   l * layerPitchBytes (rowPitchBytes between rows), its levels 1 .. at d_pyramids + l * pyramidLayerBytes + T[L].byteOffset with
 *   T[L].rowPitchBytes.  The same pixel kinds and filters by the same rules.  ONE launch per level for all layers (the layer is the
 *   grid's z; arrays of more than 65535 layers take a launch per 65535 of them).  Writes exactly the levels' bytes: not the gaps that
 *   align a level's start and not the space between layers.  A level is made with 16-byte accesses only where EVERY layer allows
 *   them: the rule of cvttmi_build_mips_device with layerPitchBytes and pyramidLayerBytes under the same test; a layer pitch that is
 *   no multiple of 16 sends level 1 of all layers through the texel-sized kernel.  CVTTMI_E_INVALID before anything is queued:
 *   what the single-image call rejects, layers == 0, layerPitchBytes below height x rowPitchBytes or no multiple of the texel,
 *   pyramidBytes below layers x pyramidLayerBytes.  levels == 1 launches nothing.
 * cvttmi_encode_texture_device: images -> packed blocks in container order, everything on hipStream: the pyramids (levels > 1),
 *   ONE tile launch for every level of every layer, one search over all tiles (groups of eight blocks are independent: the same
 *   bytes as cvttmi_encode_device per level), ONE compact launch into d_out in `order`.  The pixel kind follows the format: RGBA16F
 *   images for BC6HU / BC6HS, RGBA8 otherwise, averaged as int8 (CVTTMI_PIXELS_RGBA8_SNORM) for BC4S / BC5S; R11U / R11S have no
 *   image form and are invalid.  options / plan / allocOptions: as for cvttmi_encode_device.  d_work: caller memory on a 256-byte
 *   boundary, at least workBytes = cvttmi_texture_layout(.., that pixel kind, the format's bytes per block, ..).workBytes; it holds
 *   pyramids, tiles and padded packed blocks, its layout is private and its contents after the call are unspecified.  The library
 *   allocates and frees nothing in this call, and besides queueing the launches synchronises with nothing (BC7 orders itself after
 *   the context's previous BC7 call as cvttmi_encode_device does).  Writes exactly outBytes = blocks x bytes per block at d_out
 *   (any other outBytes is invalid) and nothing outside d_work[0, workBytes).  CVTTMI_E_INVALID before anything is queued, nothing
 *   written: what the calls above reject, NULL pointers (plan: BC7 only), a misaligned pointer. */
#define CVTTMI_ORDER_LAYER_MAJOR 0
#define CVTTMI_ORDER_LEVEL_MAJOR 1
typedef struct cvttmi_texture_sizes
{
    size_t pyramidLayerBytes, pyramidBytes;
    size_t tilesPerLayer, tiles;
    size_t blocksPerLayer, blocks;
    size_t workBytes;
} cvttmi_texture_sizes;
int cvttmi_texture_layout(uint32_t width, uint32_t height, int pixelFormat, uint32_t bytesPerBlock, uint32_t levels, uint32_t layers,
                          int order, cvttmi_texture_sizes *out);
int cvttmi_texture_subresource(uint32_t width, uint32_t height, int pixelFormat, uint32_t bytesPerBlock, uint32_t levels, uint32_t layers,
                               int order, uint32_t layer, uint32_t level, size_t *firstBlock, size_t *blockCount);
int cvttmi_build_mips_array_device(cvttmi_context *ctx, void *d_pyramids, size_t pyramidBytes, const void *d_images, uint32_t width,
                                   uint32_t height, size_t rowPitchBytes, size_t layerPitchBytes, int pixelFormat, uint32_t levels,
                                   uint32_t layers, uint32_t filter, void *hipStream);
int cvttmi_encode_texture_device(cvttmi_context *ctx, int format, void *d_out, size_t outBytes, const void *d_images, uint32_t width,
                                 uint32_t height, size_t rowPitchBytes, size_t layerPitchBytes, uint32_t layers, uint32_t levels,
                                 uint32_t filter, int order, const cvttmi_options *options, const cvttmi_bc7_plan *plan,
                                 const cvttmi_options *allocOptions, void *d_work, size_t workBytes, void *hipStream);

/* BC2 / BC3 / BC4 / BC5: cvtt::Kernels::EncodeBC2, EncodeBC3, EncodeBC4U/S, EncodeBC5U/S (reference
 * ConvectionKernels_API.cpp:101-199 -> S3TCComputer::PackRGB without alpha test, PackExplicitAlpha,
 * PackInterpolatedAlpha, ConvectionKernels_S3TC.cpp:306-715).  Input PixelBlockU8 (isSigned: PixelBlockS8, biased
 * like Util::BiasSignedInput); output 16 B per block (BC4: 8 B): BC2/BC3 = [alpha 8 B | colour 8 B], BC4 = red,
 * BC5 = [red | green].  Options used: seedPoints, refineRoundsIIC (alpha), refineRoundsS3TC + weights (colour). */
int cvttmi_encode_bc2_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks, const cvttmi_options *options, void *hipStream);
int cvttmi_encode_bc3_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks, const cvttmi_options *options, void *hipStream);
int cvttmi_encode_bc4_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks, const cvttmi_options *options, int isSigned, void *hipStream);
int cvttmi_encode_bc5_device(cvttmi_context *ctx, void *d_out, const void *d_blocks, size_t numBlocks, const cvttmi_options *options, int isSigned, void *hipStream);
int cvttmi_encode_bc2(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks, const cvttmi_options *options);
int cvttmi_encode_bc3(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks, const cvttmi_options *options);
int cvttmi_encode_bc4(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks, const cvttmi_options *options, int isSigned);
int cvttmi_encode_bc5(cvttmi_context *ctx, uint8_t *out, const uint8_t *blocks, size_t numBlocks, const cvttmi_options *options, int isSigned);

/* EAC R11: cvtt::Kernels::EncodeETC2Alpha11 (reference ConvectionKernels_API.cpp:258-268 -> CompressEACBlock,
 * ConvectionKernels_ETC.cpp:2087-2114).  blocksS16: numBlocks x PixelBlockScalarS16 (16 int16: unsigned 0..2047,
 * signed -1023..1023, clamped like the reference) -> 8 bytes per block. */
int cvttmi_encode_etc2_alpha11_device(cvttmi_context *ctx, void *d_out, const void *d_blocksS16, size_t numBlocks, int isSigned,
                                      const cvttmi_options *options, void *hipStream);
int cvttmi_encode_etc2_alpha11(cvttmi_context *ctx, uint8_t *out, const int16_t *blocksS16, size_t numBlocks, int isSigned,
                               const cvttmi_options *options);

/* ---- decoders: cvtt::Kernels::DecodeBC7 / DecodeBC6HU / DecodeBC6HS (reference
 * ConvectionKernels_API.cpp:288-310, ConvectionKernels_BC67.cpp:2206-2423, 3058-3289), batched:
 * numBlocks (multiple of 8) packed 16-byte blocks -> PixelBlockU8 (64 B) / PixelBlockF16 (128 B,
 * half bit patterns, alpha = 1.0).  Reserved modes decode like the reference (zeros). ---- */
int cvttmi_decode_bc7_device(cvttmi_context *ctx, void *d_blocks, const void *d_bc, size_t numBlocks, void *hipStream);
int cvttmi_decode_bc7(cvttmi_context *ctx, uint8_t *blocks, const uint8_t *bc, size_t numBlocks);
int cvttmi_decode_bc6h_device(cvttmi_context *ctx, void *d_blocksF16, const void *d_bc, size_t numBlocks, int isSigned, void *hipStream);
int cvttmi_decode_bc6h(cvttmi_context *ctx, uint8_t *blocksF16, const uint8_t *bc, size_t numBlocks, int isSigned);

/* ---- every format: decode, and the encoding error in one pass (not part of the reference's API) ----
 * format = CVTTMI_FMT_* (above).  A decoder writes the layout its encoder reads:
 *   BC7, BC1, BC2, BC3, ETC1, ETC2 RGB / RGBA / punch-through, EAC alpha: PixelBlockU8 (64 B; BC1 three-colour index 3 and
 *     punch-through transparent texels = (0,0,0,0); ETC RGB alpha = 255; EAC alpha = (0,0,0,a))
 *   BC4U / BC5U: PixelBlockU8 (r,0,0,255) / (r,g,0,255);  BC4S / BC5S: PixelBlockS8 (r,0,0,127) / (r,g,0,127)
 *   BC6HU / BC6HS: PixelBlockF16 (128 B, alpha 0x3C00);  R11U / R11S: PixelBlockScalarS16 (32 B, 0..2047 / -1023..1023)
 * Reconstruction follows the models the encoders score their candidates with ("Decoding and measuring").
 * The measure reads each packed block and its source once, decodes in registers and adds up the squared difference of the
 * channels the format stores (channelMask: BC1-3, BC7, ETC2 RGBA / punch-through RGBA; ETC1 / ETC2 RGB, BC6H RGB; BC5 RG;
 * BC4, R11 R; EAC A).  The source is read exactly as the encoder reads it (BC4S / BC5S: int8, -128 as -127; R11: clamped to
 * the encoder's range; BC6H: half -> float).
 * Integer formats: per block a uint32, totals uint64, exact.  BC6H: per block a float, summed in float in the order texel
 * 0..15, channel 0..2 inside; sseHdr[c] = double sums of the per-block float sums of channel c (texel 0..15), reduced in a
 * fixed order: 256 blocks per workgroup, halving tree a[i] += a[i + s] (s = 128 .. 1), one partial per workgroup, then one
 * workgroup of 1024 lanes sums a launch's partials (lane t: t, t + 1024, ... in order, then the halving tree s = 512 .. 1);
 * launches of at most 2^24 blocks
 * (host entries: chunks of 2^17) add into the totals in order.  No float atomics: the same input gives bit-identical totals
 * on every run and stream.  The partials live in one slab per context: like the BC7 hand-over list, a call on another
 * stream than the previous one waits for it (one context per stream to overlap work). ---- */
typedef struct cvttmi_error_totals
{
    uint64_t sse[4];      /* integer formats: exact per-channel sums; 0 for channels the format does not store */
    double sseHdr[4];     /* BC6H only, summation order as documented above */
    uint64_t texels;      /* texels counted per measured channel */
    uint32_t channelMask; /* bit c = channel c is measured for this format */
    int32_t format;
} cvttmi_error_totals;
/* numBlocks (multiple of 8) packed blocks -> the decoded layout above */
int cvttmi_decode_device(cvttmi_context *ctx, int format, void *d_out, const void *d_bc, size_t numBlocks, void *hipStream);
int cvttmi_decode(cvttmi_context *ctx, int format, void *out, const uint8_t *bc, size_t numBlocks);
/* d_source: numBlocks blocks of the encoder's input layout.  d_blockError: NULL, or numBlocks uint32 (float for BC6H).
 * d_totals: device memory (the host form: host memory) the totals are written to.  A call OVERWRITES all 80 bytes of the
 * totals (they need no initial value, and nothing accumulates from one call to the next) and every one of the numBlocks
 * per-block values. */
int cvttmi_measure_error_device(cvttmi_context *ctx, int format, const void *d_bc, const void *d_source, size_t numBlocks,
                                void *d_blockError, cvttmi_error_totals *d_totals, void *hipStream);
int cvttmi_measure_error(cvttmi_context *ctx, int format, const uint8_t *bc, const void *source, size_t numBlocks,
                         void *blockError, cvttmi_error_totals *totals);
/* d_bc: the ceil(W/4) x ceil(H/4) blocks, row-major, that encode_image / cvttmi_compact_rows_device produce; d_image: the
 * linear RGBA8 (every format but BC6H and R11) or RGBA16F (BC6H) image.  Texels outside width x height count nowhere. */
int cvttmi_measure_image_error_device(cvttmi_context *ctx, int format, const void *d_bc, const void *d_image, uint32_t width,
                                      uint32_t height, size_t rowPitchBytes, int pixels, void *d_blockError,
                                      cvttmi_error_totals *d_totals, void *hipStream);
/* PSNR in dB over the channels of channelMask (0 = the format's channels): 10 log10(peak^2 / MSE), peak 255 (BC4S / BC5S 254,
 * R11U 2047, R11S 2046); +inf on zero error; NaN for BC6H, for channels the format does not store and for no texels. */
double cvttmi_psnr(const cvttmi_error_totals *t, uint32_t channelMask);

/* ---- decoding into images: packed blocks as a container holds them -> linear images in HBM (not part of the reference's
 * API; the reverse of tiling, encoding and compacting rows) ----
 * d_bc: the ceil(W/4) x ceil(H/4) blocks, row-major -- any count, it need not be a multiple of 8: what encode_image,
 * cvttmi_compact_rows_device and the containers hold.  d_image: width x height texels, rowPitchBytes between rows.
 * pixels: CVTTMI_PIXELS_RGBA16F for BC6HU / BC6HS and CVTTMI_PIXELS_RGBA8 for every other format; R11U / R11S have no image
 * form.  A texel holds exactly what cvttmi_decode_device writes for it (the table under "every format"): uint8 RGBA;
 * BC4S / BC5S int8 (r,0,0,127) / (r,g,0,127); BC6H four half bit patterns, alpha 0x3C00.
 * cvttmi_decode_mips_device: d_bc holds the blocks of `levels` levels consecutively, as cvttmi_mip_layout(width, height, pixels,
 * bytes per block, levels) places them (packedByteOffset) -- what the mip containers store.  Level 0 goes to d_image
 * (rowPitchBytes between rows), levels 1 .. levels-1 into d_pyramid at the layout's byteOffset / rowPitchBytes: the mirror of
 * cvttmi_build_mips_device.  levels == 1 needs no pyramid (d_pyramid may then be NULL).  The whole chain is ONE launch.
 * Buffers.  The calls write exactly the texels of the image (images): never a byte before or behind them, between the end of
 * a row and the next pitch, or in the gaps that align a level's start, whatever the edge blocks hold beyond width x height.
 * d_image / d_pyramid: aligned to the texel (4 / 8 bytes); rowPitchBytes a multiple of the texel and at least one row; d_bc:
 * min(bytes per block, 16).  Where an image's first texel and its pitch are both multiples of 16 bytes (per level, for a
 * chain: the small levels have 4- or 8-byte pitches), the rows of every block that lies wholly inside the image are stored 16
 * bytes at a time; blocks cut by the right or bottom edge, and every block of an image that is not so aligned, texel by texel.
 * CVTTMI_E_INVALID before anything is queued, nothing written: NULL pointers, a zero size, an unknown format id or R11, a
 * pixel kind that is not the format's (CVTTMI_PIXELS_RGBA8_SNORM included), rowPitchBytes below the row or no multiple of the
 * texel, a misaligned pointer, levels 0 or above cvttmi_mip_level_count, pyramidBytes below the layout's, 2^32 blocks or more.
 * Both calls are simply queued on the stream given (no context work space); images, pyramid and blocks must not overlap.
 * Device pointers only. */
int cvttmi_decode_image_device(cvttmi_context *ctx, int format, void *d_image, size_t rowPitchBytes, int pixels,
                               const void *d_bc, uint32_t width, uint32_t height, void *hipStream);
int cvttmi_decode_mips_device(cvttmi_context *ctx, int format, void *d_image, size_t rowPitchBytes,
                              void *d_pyramid, size_t pyramidBytes, int pixels, const void *d_bc,
                              uint32_t width, uint32_t height, uint32_t levels, void *hipStream);

/* ---- one job on several devices (csrc/multi.cpp).  The north-star's "large images shard by block row across the GPUs of one
 * node", for callers of this C interface (the reference has no counterpart: its callers parallelise by threads over groups,
 * etc2packer.cpp:215-281).  Groups of 8 blocks are independent, so the search needs no exchange: the job is cut into
 * contiguous ranges of whole block rows, moved to the next group boundary where a row is no multiple of 8 blocks
 * (cvttmi_shard_block_rows -- the same rule as convectionkernels_amd/sharding.py), each range is encoded by its own context on
 * its own device from its own host thread, and the packed blocks land in `out` at the range's offset.  Output bytes equal the
 * single-device call's.  `devices` may name a device more than once (a context each).  blocksPerRow = blocks in one block row of
 * the tiled image (ceil(ceil(w/4)/8)*8, cvttmi_tiled_block_count); 0 = no rows, shard by groups.
 * cvttmi_multi_*: a handle owning one context per list entry.  A handle runs ONE job at a time (a mutex; the setters take it
 * too): concurrent callers of one handle -- including the C++ face's *Batch calls, which share the handle of the drop-in's device
 * list -- are serialised; use a handle per worker thread to overlap jobs.
 * cvttmi_encode_*_multi: stateless forms.  They keep one handle (contexts, staging) per distinct device list FOR THE LIFE OF THE
 * PROCESS -- nothing is released before exit -- and report failures through cvttmi_multi_last_error(NULL): the text of the calling
 * thread's most recent failed multi-device call.
 * No call of this section lets a C++ exception out; allocation failures come back as CVTTMI_E_HIP.
 * Between processes (one per GPU) the packed output is gathered with RCCL send/recv over xGMI instead: sharding.py,
 * bench.py --gpus N. ---- */
typedef struct cvttmi_multi cvttmi_multi;
int cvttmi_shard_block_rows(size_t blockRows, size_t blocksPerRow, int rank, int world, size_t *firstBlock, size_t *lastBlock);
int cvttmi_multi_create(cvttmi_multi **out, const int *devices, int numDevices);
void cvttmi_multi_destroy(cvttmi_multi *m);
const char *cvttmi_multi_last_error(const cvttmi_multi *m);
int cvttmi_multi_num_devices(const cvttmi_multi *m);
cvttmi_context *cvttmi_multi_context(cvttmi_multi *m, int index);
int cvttmi_multi_last_shard(const cvttmi_multi *m, int index, size_t *firstBlock, size_t *lastBlock);
int cvttmi_multi_set_rcp_table(cvttmi_multi *m, const float lut[17]);
int cvttmi_multi_set_exhaustive(cvttmi_multi *m, int exhaustive);
/* format = CVTTMI_FMT_*: every format of the table (cvttmi_format_info gives the sizes; each shard is one cvttmi_encode /
 * cvttmi_encode_device call on its context, so what those accept is accepted here -- all seventeen ids, where this section
 * took six before).  plan: BC7 only (NULL otherwise); the ETC2 formats take the chroma axes from `options`.  Host buffers
 * (page-locked ones are transferred in place). */
int cvttmi_multi_encode(cvttmi_multi *m, int format, uint8_t *out, const uint8_t *blocks, size_t numBlocks, size_t blocksPerRow,
                        const cvttmi_options *options, const cvttmi_bc7_plan *plan);
/* Device-resident callers (the tiling kernel or an upload of the caller's own has put every shard where it is searched):
 * d_shards[r] = HBM pointer ON devices[r] to the PixelBlocks of shard r, i.e. blocks [first_r, last_r) of the job as
 * cvttmi_shard_block_rows(numBlocks / blocksPerRow, blocksPerRow, r, numDevices) cuts it (NULL allowed for an empty shard);
 * d_out = numBlocks packed blocks ON devices[0].  Every device searches its shard on a stream of its own; shards on the root
 * device write their slice of d_out directly, the others write a buffer on their own device that is then copied into the slice
 * with hipMemcpyPeerAsync -- over xGMI, with peer access enabled where the pair allows it: the north-star's gather of the packed
 * output for a single process.  Returns when d_out is complete.  (CVTTMI_MULTI_FORCE_STAGE=1 in the environment when the handle is
 * created sends root-device shards through the staged route too: how a one-GPU box tests it.) */
int cvttmi_multi_encode_device(cvttmi_multi *m, int format, void *d_out, const void *const *d_shards, size_t numBlocks, size_t blocksPerRow,
                               const cvttmi_options *options, const cvttmi_bc7_plan *plan);
int cvttmi_encode_bc7_multi(const int *devices, int numDevices, uint8_t *out, const uint8_t *blocks, size_t numBlocks, size_t blocksPerRow,
                            const cvttmi_options *options, const cvttmi_bc7_plan *plan);
int cvttmi_encode_bc1_multi(const int *devices, int numDevices, uint8_t *out, const uint8_t *blocks, size_t numBlocks, size_t blocksPerRow,
                            const cvttmi_options *options);
int cvttmi_encode_bc6h_multi(const int *devices, int numDevices, uint8_t *out, const uint8_t *blocks, size_t numBlocks, size_t blocksPerRow,
                             const cvttmi_options *options, int isSigned);
int cvttmi_encode_etc2_rgba_multi(const int *devices, int numDevices, uint8_t *out, const uint8_t *blocks, size_t numBlocks, size_t blocksPerRow,
                                  const cvttmi_options *options);
/* The device list of the C++ face's *Batch entry points (cvtt::Kernels::EncodeBC7Batch, EncodeBC1Batch, EncodeBC6HU/SBatch,
 * EncodeETC2RGBABatch): more than one entry = calls of at least 65 536 blocks are sharded over the list as above (by groups).
 * Default: the environment variable CVTTMI_DEVICES ("0,1,2,3"), else the single device CVTTMI_DEVICE (default 0).
 * Configuration call: not to be made while another thread is inside a *Batch call (it replaces the handle those calls use). */
int cvttmi_dropin_set_devices(const int *devices, int numDevices);

/* Arithmetic self-test: evaluates binary32 divide and square root on `count` pseudo-random finite
 * operand patterns (zeros, denormals and both signs included) with the expressions and compiler
 * flags the encoders use, and counts results that differ from the host's DIVSS / SQRTSS -- the
 * arithmetic contract behind bit-exactness (reference ParallelMath.h:261-323, 959-965). */
int cvttmi_selftest_arith(cvttmi_context *ctx, uint64_t count, uint64_t seed, uint64_t *divMismatches, uint64_t *sqrtMismatches);

/* Time (ms, HIP events on the launch stream) and count of the encode and decode calls since timing
 * was last enabled: each *_device call counts once, a host-pointer call once per launch of its pipeline. */
int cvttmi_timing_enable(cvttmi_context *ctx, int enable);
int cvttmi_timing_read(cvttmi_context *ctx, double *totalMs, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif
