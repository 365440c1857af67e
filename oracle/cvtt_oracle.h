/* TEST INFRASTRUCTURE ONLY -- CPU restatement of the reference's per-block encoders.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load the
 * library built from this file.  The product path (convectionkernels_amd/) never does.
 *
 * Parity status: PINNED.  Every function here is checked bit-for-bit against the real
 * reference compiled from /root/reference (oracle/_ref, see oracle/Makefile) and against
 * the committed golden vectors under tests/golden/ (tests/test_oracle_*.py).
 */
#ifndef CVTT_ORACLE_H
#define CVTT_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Byte-compatible images of the reference PODs (ConvectionKernels.h:73-103, 142-199). */
typedef struct orc_options
{
    uint32_t flags;
    float threshold;
    float redWeight, greenWeight, blueWeight, alphaWeight;
    int32_t refineRoundsBC7, refineRoundsBC6H, refineRoundsIIC, refineRoundsS3TC;
    int32_t seedPoints;
} orc_options;

typedef struct orc_bc7_plan
{
    uint64_t mode1PartitionEnabled;
    uint64_t mode2PartitionEnabled;
    uint64_t mode3PartitionEnabled;
    uint16_t mode0PartitionEnabled;
    uint64_t mode7RGBAPartitionEnabled;
    uint64_t mode7RGBPartitionEnabled;
    uint8_t mode4SP[4][2];
    uint8_t mode5SP[4];
    uint8_t mode6Enabled; /* C++ bool */
    uint8_t seedPointsForShapeRGB[243];
    uint8_t seedPointsForShapeRGBA[129];
    uint8_t rgbaShapeList[129];
    uint8_t rgbaNumShapesToEvaluate;
    uint8_t rgbShapeList[243];
    uint8_t rgbNumShapesToEvaluate;
} orc_bc7_plan;

enum
{
    ORC_FLAG_BC7_FAST_INDEXING = 0x008,
    ORC_FLAG_BC7_TRY_SINGLE_COLOR = 0x010,
    ORC_FLAG_BC7_RESPECT_PUNCHTHROUGH = 0x020,
    ORC_FLAG_BC6H_FAST_INDEXING = 0x040,
    ORC_FLAG_S3TC_EXHAUSTIVE = 0x080,
    ORC_FLAG_S3TC_PARANOID = 0x100,
    ORC_FLAG_UNIFORM = 0x200
};

size_t orc_sizeof_options(void);
size_t orc_sizeof_bc7_plan(void);

/* rcpps(i) for i = 1..16 on this host (entry 0 = entry 1); SURVEY App. A. */
void orc_probe_rcp(float out17[17]);

/* Group g = blocks [8g, 8g+8).  numBlocks must be a multiple of 8.
 * rcp17: the 17-entry reciprocal table to use (NULL = probe this host).
 * threads: worker threads over groups (<=1: run inline).
 * Returns 0, or a negative value for unsupported flag combinations. */
int orc_encode_bc7(uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                   const orc_options *options, const orc_bc7_plan *plan,
                   const float *rcp17, int threads);

int orc_encode_bc1(uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                   const orc_options *options, const float *rcp17, int threads);

/* blocksF16: numBlocks * 128 bytes of PixelBlockF16 (half bits as int16, RGBA; alpha ignored). */
int orc_encode_bc6h(uint8_t *out, const uint8_t *blocksF16, size_t numBlocks,
                    const orc_options *options, int isSigned, const float *rcp17, int threads);

/* mode 0: ETC2 RGB (8 B/block), 1: ETC2 RGBA = [EAC alpha | colour] (16 B/block), 2: EAC alpha (8 B/block) */
int orc_encode_etc2(uint8_t *out, const uint8_t *blocks, size_t numBlocks,
                    const orc_options *options, int mode, int threads);
/* the same with the Options of AllocETC2Data given apart (their colour weights fix the chroma axes, ETC.cpp:3117-3145) */
int orc_encode_etc2_alloc(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                          const orc_options *allocOptions, int mode, int threads);

/* BC2 / BC3 / BC4U / BC4S / BC5U / BC5S (format 2..7; signed formats take PixelBlockS8): 8 B (BC4) or 16 B per block */
int orc_encode_s3tc(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, int format,
                    const float *rcp17, int threads);

/* EAC R11 (cvtt::Kernels::EncodeETC2Alpha11): numBlocks * 16 int16 (PixelBlockScalarS16) -> 8 B/block */
int orc_encode_eac11(uint8_t *out, const int16_t *blocksS16, size_t numBlocks, int isSigned);

/* The same encodes (same bytes), also writing each block's final error -- the score of the candidate that is emitted --
 * into caller-supplied arrays indexed by block (NULL = not wanted).
 *   colorErr: one float per block: BC1, BC2 / BC3 colour, ETC1 and ETC2 colour (modes 0, 1, 3, 4)
 *   alphaErr: s3tc: one float per block and interpolated channel (BC3, BC4: 1; BC5: 2; BC2 keeps none)
 *             etc2: one uint32 per block, the EAC alpha error (modes 1, 2) */
int orc_encode_bc1_err(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                       const float *rcp17, int threads, float *err);
int orc_encode_s3tc_err(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options, int format,
                        const float *rcp17, int threads, float *colorErr, float *alphaErr);
int orc_encode_etc2_err(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                        const orc_options *allocOptions, int mode, int threads, float *colorErr, uint32_t *alphaErr);

/* ---- the small ETC functions one at a time (cvtt_oracle_etc_parts.inc; the parts, variants and domains: etc_parts.h) ----
 * chunks [firstChunk, firstChunk + numChunks) of a sweep: checksums, results in full (either may be NULL) and the count of
 * results that carry ETCP_FLAG; or the results of listed inputs.  -1: no such part, chunk or input. */
int orc_etc_parts(int part, int variant, const float *weights3, const int32_t *table, uint32_t firstChunk, uint32_t numChunks,
                  uint64_t *sums, uint32_t *full, uint64_t *flagged, int threads);
int orc_etc_parts_at(int part, int variant, const float *weights3, const int32_t *table, const uint32_t *inputs, size_t count, uint32_t *out);

/* ---- group-coupling site switch (tests/test_group_coupling.py, tools/find_coupling_witnesses.py) ----
 * Each bit makes ONE semantic AnySet / AllSet site of SURVEY App. B behave the way an encoder that got it wrong would:
 * the horizontal test sees the block's own flag (or count) only, never its seven group mates'.  Block l of a group is
 * then what a group encode gives for l when every masked horizontal test is answered with l's own value, so all the
 * other coupling stays exactly as it is.  siteMask == 0 is the plain entry point, byte for byte. */
enum
{
    ORC_SITE_BC7_ANY_ALPHA = 1 << 0,      /* anyBlockHasAlpha, BC67.cpp:1066-1069: own minAlpha < 255 */
    ORC_SITE_BC7_ALLOW_RGB = 1 << 1,      /* allowRGBModes, BC67.cpp:1072: own minAlpha > 250 */
    ORC_SITE_BC7_PUNCH_COMMIT = 1 << 2,   /* the AnySet / AllSet guards of the commit rule, BC67.cpp:1300-1303, 1406-1428: own flags */
    ORC_SITE_BC6H_DUP_SKIP = 1 << 3,      /* AllSet(anySame), BC67.cpp:2868-2876: own anySame (the own round is dropped, refiner left empty) */
    ORC_SITE_BC6H_COMMIT_LOOP = 1 << 4,   /* AnySet(errorBetter / needsCommit), BC67.cpp:2936-2984: own flags */
    ORC_SITE_ETC2_OPAQUE_TMAX = 1 << 5,   /* opaque T mode: maxUniqueColors, ETC.cpp:563-584: own count (slot H2 never read) */
    ORC_SITE_ETC2_PUNCH_TMAX = 1 << 6,    /* virtual T mode: clusterMaxLine and maxUniqueColors, ETC.cpp:1036-1142: own counts */
    ORC_SITE_ETC2_PUNCH_ALPHA = 1 << 7,   /* AllSet(allTransparent) / AnySet(anyTransparent), ETC.cpp:1705-1867: own flags */
    ORC_SITE_BC1_TEST_COUNTS = 1 << 8,    /* TestCounts' escape on the group's largest element count, S3TC.cpp:275-290: own count */
    ORC_SITE_COUNT = 9
};

int orc_encode_bc7_sites(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                         const orc_bc7_plan *plan, const float *rcp17, int threads, uint32_t siteMask);
int orc_encode_bc1_sites(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                         const float *rcp17, int threads, uint32_t siteMask);
int orc_encode_bc6h_sites(uint8_t *out, const uint8_t *blocksF16, size_t numBlocks, const orc_options *options,
                          int isSigned, const float *rcp17, int threads, uint32_t siteMask);
int orc_encode_etc2_sites(uint8_t *out, const uint8_t *blocks, size_t numBlocks, const orc_options *options,
                          const orc_options *allocOptions, int mode, int threads, uint32_t siteMask);

#ifdef __cplusplus
}
#endif
#endif
