// Resize to any size (include/cvtt_mi355x.h, "resize"): the Q14 two-pass rule of the mip kernels with one weight row per output
// column and per output row.  RGBA8 and RGBA8_SNORM texels; the plain rule, SRGB and NORMAL; clamp, repeat and mirror.  (RGBA16F:
// the plain rule in float -- resample_common.h, "RGBA16F" -- as KIND = kRGBA16F of the same three kernel templates: 8-byte texels,
// an entry the four float sums, the same routes, tables and work space.)  The tables
// (cvttmi_resize_taps: weights and first taps of both axes) lie in device memory, in the caller's work space:
//   wx[k * dstW + x]  the weight of tap k of output column x (tap-major: the lanes of a wave read neighbouring columns)
//   fx[x]             the unwrapped source column of its tap 0
//   wy[y * ny + k], fy[y]  the same for output row y (row-major: a wave works on one row, the weight is the same for all its lanes)
// The two passes, the layer in the grid's z:
//   horizontal  entry (x, r), r a SOURCE row: h' of output column x from the nx taps of row r.  A lane walks its taps through
//               the wrap with 4-byte reads; neighbouring lanes read overlapping texels (L1 / L2).
//   vertical    output texel (x, y) from the ny entries (x, fy[y] + k), the row wrapped; one 4-byte store.
// An entry is: plain int16 x 4; SRGB int32 x 4 (channel 3 the plain h'); NORMAL int16 x 4 of X and alpha plus int16 x 4 of the
// plain bytes, which the vertical pass reads only where the three sums of X are all zero.
// One launch where the footprint allows it (cvttmi_resize_fused_rows): a workgroup of 256 lanes owns a tile of kTileX x kTileY
// output texels and keeps the entries of the source rows under it, fy[y0] .. fy[y1] + ny - 1, in LDS sized per launch (at most
// kFusedLdsBytes with the sRGB tables).  Two launches otherwise, a workgroup on 256 columns of kRows neighbouring rows and the
// entries of the whole image (dstW x srcH per layer) in the work space: nothing there depends on the ratio, a footprint of any
// length is a loop.  The sRGB tables are copied to LDS once per workgroup (5.5 KB vertical, 0.5 KB horizontal).  No scratch.
// Every product is a 24-bit multiply: |tap| <= 16385 + what a row is missing, a value or an h' below 2^17 (sRGB: T <= 65535,
// |h'| <= (65535 P + 8192) >> 14 < 2^17 for the P < 2^15 that cvttmi_resize_taps lets through), and that function has checked that
// the sums stay inside int32.
#include "resample_common.h"
#include "cvtt_launchers.h"

namespace
{
enum
{
    kRows = 8,  // two launches: rows of one workgroup
    kTileX = 64, // one launch: the tile of output texels of a workgroup
    kTileY = 16,
    kFusedLdsBytes = 52 * 1024 // ... and the LDS it may take: three workgroups share a CU's 160 KB
};

struct NormalEntry
{
    short4 n, p; // h' of X (channels 0..2) and of alpha; h' of the plain bytes of channels 0..2
};

// what the pixel kind (and the rule) decide: the texel of an image and the entry between the passes
template <int KIND>
struct TexelOf
{
    typedef typename std::conditional<KIND == kRGBA16F, uint2, uint32_t>::type type;
};

template <int KIND, int RULE>
struct EntryOf
{
    typedef typename std::conditional<RULE == kSrgb, int4, typename std::conditional<RULE == kNormal, NormalEntry, short4>::type>::type Integer;
    typedef typename std::conditional<KIND == kRGBA16F, float4, Integer>::type type;
};

struct ResizeArgs
{
    const uint8_t *src;
    uint8_t *dst;
    void *mid; // two launches: the intermediate, dstW x srcH entries per layer, layers consecutive
    size_t srcPitch, srcLayer, dstPitch, dstLayer;
    uint32_t srcW, srcH, dstW, dstH;
    const int16_t *wx, *wy;
    const int32_t *fx, *fy;
    uint32_t nx, ny, wrap;
};

// The horizontal pass of one entry: output column x of one source row.  tap: the column's weights, `stride` apart.
template <int KIND, int RULE>
__device__ __forceinline__ typename EntryOf<KIND, RULE>::type horizontalEntry(const ResizeArgs &a, const typename TexelOf<KIND>::type *row,
                                                                              int32_t first, const int16_t *tap, uint32_t stride,
                                                                              const uint16_t *lin)
{
    Walk w = walkFrom(first, a.srcW, a.wrap);
    if constexpr (KIND == kRGBA16F)
    {
        float h[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t k = 0; k < a.nx; k++, tap += stride)
        {
            const uint2 texel = row[walkIndex(w)];
            walkStep(w);
            const float q = static_cast<float>(*tap) * (1.0f / 16384.0f);
            h[0] = h[0] + q * halfValue(texel.x);
            h[1] = h[1] + q * halfValue(texel.x >> 16);
            h[2] = h[2] + q * halfValue(texel.y);
            h[3] = h[3] + q * halfValue(texel.y >> 16);
        }
        return make_float4(h[0], h[1], h[2], h[3]);
    }
    else
    {
        int h[7] = {0, 0, 0, 0, 0, 0, 0}; // 0..2: the colour channels under the rule; 3: alpha; 4..6 (NORMAL): the plain bytes of 0..2
        for (uint32_t k = 0; k < a.nx; k++, tap += stride)
        {
            const uint32_t texel = row[walkIndex(w)];
            walkStep(w);
            const int q = *tap;
#pragma unroll
            for (int c = 0; c < 4; c++)
            {
                // ruleValue of c and, under NORMAL, of 4 + c, spelled out: through the function the NORMAL instances order their
                // instructions differently
                const uint32_t v = (texel >> (8 * c)) & 255u;
                const int plain = KIND == kRGBA8Snorm ? static_cast<int>(static_cast<int8_t>(v)) : static_cast<int>(v);
                int value = plain;
                if (c < 3 && RULE == kSrgb)
                    value = lin[v];
                if (c < 3 && RULE == kNormal)
                {
                    value = KIND == kRGBA8Snorm ? max(plain, -127) : 2 * plain - 255;
                    h[4 + c] += __mul24(q, plain);
                }
                h[c] += __mul24(q, value);
            }
        }
        const int h3 = (h[3] + 512) >> 10;
        if constexpr (RULE == kSrgb)
            return make_int4((h[0] + (1 << 13)) >> 14, (h[1] + (1 << 13)) >> 14, (h[2] + (1 << 13)) >> 14, h3);
        else
        {
            const short4 e = make_short4((short)((h[0] + 512) >> 10), (short)((h[1] + 512) >> 10), (short)((h[2] + 512) >> 10), (short)h3);
            if constexpr (RULE == kNormal)
                return NormalEntry{e, make_short4((short)((h[4] + 512) >> 10), (short)((h[5] + 512) >> 10), (short)((h[6] + 512) >> 10), 0)};
            else
                return e;
        }
    }
}

// The vertical pass of one output texel: at(k) = the entry under tap k, tap[k] its weight; lo: the lower clamp of RGBA16F.
template <int KIND, int RULE, class At>
__device__ __forceinline__ typename TexelOf<KIND>::type verticalTexel(const int16_t *tap, uint32_t ny, const SrgbEncodeTables &tables, float lo, At at)
{
    if constexpr (KIND == kRGBA16F)
    {
        float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (uint32_t k = 0; k < ny; k++)
        {
            const float q = static_cast<float>(tap[k]) * (1.0f / 16384.0f);
            const float4 e = at(k);
            s[0] = s[0] + q * e.x;
            s[1] = s[1] + q * e.y;
            s[2] = s[2] + q * e.z;
            s[3] = s[3] + q * e.w;
        }
        return rangedTexel(s, lo);
    }
    else
    {
        int s[4] = {0, 0, 0, 0};
        for (uint32_t k = 0; k < ny; k++)
        {
            const int q = tap[k];
            short4 e16;
            int4 e32;
            if constexpr (RULE == kSrgb)
                e32 = at(k);
            else if constexpr (RULE == kNormal)
                e16 = at(k).n;
            else
                e16 = at(k);
            s[0] += __mul24(q, RULE == kSrgb ? e32.x : (int)e16.x);
            s[1] += __mul24(q, RULE == kSrgb ? e32.y : (int)e16.y);
            s[2] += __mul24(q, RULE == kSrgb ? e32.z : (int)e16.z);
            s[3] += __mul24(q, RULE == kSrgb ? e32.w : (int)e16.w);
        }
        uint32_t out = plainByte<KIND>(s[3]) << 24;
        if constexpr (RULE == kPlain)
        {
#pragma unroll
            for (int c = 0; c < 3; c++)
                out |= plainByte<KIND>(s[c]) << (8 * c);
        }
        else if constexpr (RULE == kSrgb)
        {
#pragma unroll
            for (int c = 0; c < 3; c++)
                out |= srgbEncode(tables, static_cast<uint32_t>(min(max((s[c] + (1 << 11)) >> 12, 0), 4 * 65535))) << (8 * c);
        }
        else
        {
            const int S[3] = {(s[0] + 128) >> 8, (s[1] + 128) >> 8, (s[2] + 128) >> 8};
            if ((S[0] | S[1] | S[2]) == 0)
            {
                int p[3] = {0, 0, 0};
                for (uint32_t k = 0; k < ny; k++)
                {
                    const short4 e = at(k).p;
                    const int q = tap[k];
                    p[0] += __mul24(q, e.x);
                    p[1] += __mul24(q, e.y);
                    p[2] += __mul24(q, e.z);
                }
#pragma unroll
                for (int c = 0; c < 3; c++)
                    out |= plainByte<KIND>(p[c]) << (8 * c);
            }
            else
            {
                const float fx = static_cast<float>(S[0]), fy = static_cast<float>(S[1]), fz = static_cast<float>(S[2]);
                const float f[3] = {fx, fy, fz};
                const float len = sqrtf((fx * fx + fy * fy) + fz * fz); // (every operation rounds on its own: -ffp-contract=off)
#pragma unroll
                for (int c = 0; c < 3; c++)
                    out |= normalByte<KIND>(f[c] / len) << (8 * c);
            }
        }
        return out;
    }
}

// ---- one launch: a tile of kTileX x kTileY output texels per workgroup, the two passes separated through LDS ----
// The source rows under a tile are fy[y0] .. fy[y1] + ny - 1 (fy does not decrease); `rows` of them at most, over all tiles.
template <int KIND, int RULE>
__global__ void __launch_bounds__(256) cvttmi_resize_fused_kernel(ResizeArgs a, uint32_t rows, float lo)
{
    typedef typename TexelOf<KIND>::type Texel;
    typedef typename EntryOf<KIND, RULE>::type Entry;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    Entry *hbuf = reinterpret_cast<Entry *>(lds); // rows x kTileX entries
    __shared__ SrgbEncodeTables tables;           // (no LDS is allocated where it is not read)
    __shared__ uint16_t lin[RULE == kSrgb ? 256 : 1];
    if constexpr (RULE == kSrgb)
    {
        loadLinear(lin);
        loadEncode(tables);
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x, x = lane & (kTileX - 1), x0 = blockIdx.x * kTileX, y0 = blockIdx.y * kTileY;
    const uint32_t tileH = min(a.dstH - y0, (uint32_t)kTileY);
    const bool inside = x0 + x < a.dstW;
    const int32_t top = a.fy[y0];
    const uint32_t used = static_cast<uint32_t>(a.fy[y0 + tileH - 1] - top) + a.ny; // <= rows: the host has looked at every tile
    if (inside && used <= rows)
    {
        const int32_t first = a.fx[x0 + x];
        const int16_t *tap = a.wx + x0 + x;
        Walk wy = walkFrom((int64_t)top + (lane / kTileX), a.srcH, a.wrap);
        for (uint32_t r = lane / kTileX; r < used; r += 256u / kTileX)
        {
            const Texel *row = reinterpret_cast<const Texel *>(a.src + blockIdx.z * a.srcLayer + (size_t)walkIndex(wy) * a.srcPitch);
            hbuf[r * kTileX + x] = horizontalEntry<KIND, RULE>(a, row, first, tap, a.dstW, lin);
#pragma unroll
            for (uint32_t i = 0; i < 256u / kTileX; i++)
                walkStep(wy);
        }
    }
    __syncthreads();
    if (inside && used <= rows)
    {
        const uint32_t yg = lane / kTileX;
        for (uint32_t j = 0; j < (uint32_t)kTileY / (256u / kTileX); j++)
        {
            const uint32_t y = y0 + yg * (kTileY / (256u / kTileX)) + j;
            if (y >= y0 + tileH)
                break;
            const Entry *column = hbuf + static_cast<uint32_t>(a.fy[y] - top) * kTileX + x;
            const Texel out = verticalTexel<KIND, RULE>(a.wy + (size_t)y * a.ny, a.ny, tables, lo, [&](uint32_t k) { return column[k * kTileX]; });
            reinterpret_cast<Texel *>(a.dst + blockIdx.z * a.dstLayer + (size_t)y * a.dstPitch)[x0 + x] = out;
        }
    }
}

// ---- two launches: any footprint ----
template <int KIND, int RULE>
__global__ void __launch_bounds__(256) cvttmi_resize_h_kernel(ResizeArgs a)
{
    typedef typename TexelOf<KIND>::type Texel;
    typedef typename EntryOf<KIND, RULE>::type Entry;
    __shared__ uint16_t lin[RULE == kSrgb ? 256 : 1];
    if constexpr (RULE == kSrgb)
    {
        loadLinear(lin);
        __syncthreads();
    }
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.dstW)
        return;
    const int32_t first = a.fx[x];
    const uint32_t r0 = blockIdx.y * kRows, r1 = min(r0 + kRows, a.srcH);
    Entry *mid = static_cast<Entry *>(a.mid) + ((size_t)blockIdx.z * a.srcH + r0) * a.dstW + x;
    for (uint32_t r = r0; r < r1; r++, mid += a.dstW)
    {
        const Texel *row = reinterpret_cast<const Texel *>(a.src + blockIdx.z * a.srcLayer + (size_t)r * a.srcPitch);
        *mid = horizontalEntry<KIND, RULE>(a, row, first, a.wx + x, a.dstW, lin);
    }
}

template <int KIND, int RULE>
__global__ void __launch_bounds__(256) cvttmi_resize_v_kernel(ResizeArgs a, float lo)
{
    typedef typename TexelOf<KIND>::type Texel;
    typedef typename EntryOf<KIND, RULE>::type Entry;
    __shared__ SrgbEncodeTables tables; // (no LDS is allocated where it is not read)
    if constexpr (RULE == kSrgb)
    {
        loadEncode(tables);
        __syncthreads();
    }
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.dstW)
        return;
    const Entry *mid = static_cast<const Entry *>(a.mid) + (size_t)blockIdx.z * a.srcH * a.dstW + x;
    const uint32_t y0 = blockIdx.y * kRows, y1 = min(y0 + kRows, a.dstH);
    for (uint32_t y = y0; y < y1; y++)
    {
        const int32_t first = a.fy[y];
        // (the walk starts anew for the second loop of a NORMAL texel whose sums are zero: k counts up from 0 both times.  Only
        // NORMAL needs it; every integer kind carries it, which is the code these kernels have always had: docs/history.md)
        Walk w = walkFrom(first, a.srcH, a.wrap);
        const Texel out = verticalTexel<KIND, RULE>(a.wy + (size_t)y * a.ny, a.ny, tables, lo, [&](uint32_t k) {
            if (KIND != kRGBA16F && k == 0)
                w = walkFrom(first, a.srcH, a.wrap);
            const Entry e = mid[(size_t)walkIndex(w) * a.dstW];
            walkStep(w);
            return e;
        });
        reinterpret_cast<Texel *>(a.dst + blockIdx.z * a.dstLayer + (size_t)y * a.dstPitch)[x] = out;
    }
}

template <int KIND, int RULE>
hipError_t launchResize(const ResizeArgs &a, uint32_t layers, uint32_t fusedRows, float lo, hipStream_t stream)
{
    if (fusedRows)
    {
        const dim3 grid((a.dstW + kTileX - 1u) / kTileX, (a.dstH + kTileY - 1u) / kTileY, layers);
        hipLaunchKernelGGL((cvttmi_resize_fused_kernel<KIND, RULE>), grid, dim3(256),
                           (size_t)fusedRows * kTileX * sizeof(typename EntryOf<KIND, RULE>::type), stream, a, fusedRows, lo);
        return hipGetLastError();
    }
    const uint32_t gx = (a.dstW + 255u) / 256u;
    hipLaunchKernelGGL((cvttmi_resize_h_kernel<KIND, RULE>), dim3(gx, (a.srcH + kRows - 1u) / kRows, layers), dim3(256), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL((cvttmi_resize_v_kernel<KIND, RULE>), dim3(gx, (a.dstH + kRows - 1u) / kRows, layers), dim3(256), 0, stream, a, lo);
    return hipGetLastError();
}
} // namespace

// bytes of one entry of the intermediate of a pixel kind under a rule (0: no such pair)
extern "C" size_t cvttmi_resize_entry_bytes(int kind, uint32_t rule)
{
    size_t bytes = 0;
    const hipError_t e = withKindRule(kind, rule, [&](auto k, auto r) {
        bytes = sizeof(typename EntryOf<k(), r()>::type);
        return hipSuccess;
    });
    return e == hipSuccess ? bytes : 0;
}

// The path of a resize, from the first taps of its dstH output rows (ny taps each): the most source rows under one tile where
// they fit in kFusedLdsBytes of LDS next to the sRGB tables -- one launch --, else 0 -- two launches.  Host only.
extern "C" uint32_t cvttmi_resize_fused_rows(int kind, uint32_t rule, const int32_t *first, uint32_t dstH, uint32_t ny)
{
    const size_t entry = cvttmi_resize_entry_bytes(kind, rule);
    const size_t room = kFusedLdsBytes - (rule == kSrgb ? sizeof(SrgbEncodeTables) + 512u : 0u);
    uint64_t rows = 0;
    for (uint32_t y0 = 0; y0 < dstH; y0 += kTileY)
    {
        const uint32_t y1 = dstH - y0 < (uint32_t)kTileY ? dstH - 1u : y0 + kTileY - 1u;
        const uint64_t used = (uint64_t)((int64_t)first[y1] - first[y0]) + ny;
        rows = used > rows ? used : rows;
    }
    return entry && rows * kTileX * entry <= room ? static_cast<uint32_t>(rows) : 0u;
}

// `layers` images (1 .. 65535, sizes 1 .. 65535) resized under `rule` = CVTTMI_MIP_FILTER_BOX (the plain rule), _SRGB or _NORMAL and
// `wrap` = 0 or one CVTTMI_MIP_WRAP_* flag.  d_wx (tap-major), d_fx, d_wy (row-major), d_fy: the tables, in device memory.
// fusedRows = cvttmi_resize_fused_rows of d_fy's values; where it is 0, d_mid holds layers x srcH x dstW entries of
// cvttmi_resize_entry_bytes(kind, rule), on a 16-byte boundary.  `range`: one CVTTMI_MIP_HDR_* flag for RGBA16F, 0 otherwise.
extern "C" hipError_t cvttmi_launch_resize(const void *d_src, size_t srcPitch, size_t srcLayer, uint32_t srcW, uint32_t srcH, void *d_dst,
                                           size_t dstPitch, size_t dstLayer, uint32_t dstW, uint32_t dstH, uint32_t layers, int kind,
                                           uint32_t rule, uint32_t wrap, uint32_t range, const int16_t *d_wx, const int32_t *d_fx, uint32_t nx,
                                           const int16_t *d_wy, const int32_t *d_fy, uint32_t ny, void *d_mid, uint32_t fusedRows,
                                           hipStream_t stream)
{
    if (!mipLayersOk(layers) || srcW == 0 || srcH == 0 || dstW == 0 || dstH == 0 || (srcW | srcH | dstW | dstH) > 65535u || nx == 0 || ny == 0 ||
        !wrapOk(wrap) || !d_wx || !d_fx || !d_wy || !d_fy || (!fusedRows && !d_mid) ||
        (size_t)fusedRows * kTileX * cvttmi_resize_entry_bytes(kind, rule) > kFusedLdsBytes || !rangeFitsKind(kind, range))
        return hipErrorInvalidValue;
    const ResizeArgs a = {static_cast<const uint8_t *>(d_src), static_cast<uint8_t *>(d_dst), d_mid, srcPitch, srcLayer, dstPitch, dstLayer,
                          srcW, srcH, dstW, dstH, d_wx, d_wy, d_fx, d_fy, nx, ny, wrap};
    return withKindRule(kind, rule, [&](auto k, auto r) { return launchResize<k(), r()>(a, layers, fusedRows, hdrRangeLow(range), stream); });
}
