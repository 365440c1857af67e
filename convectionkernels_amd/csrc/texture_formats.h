// One row per format id (include/cvtt_mi355x.h, CVTTMI_FMT_*) with every fact the decode / measure path and the shim need of a
// format; nothing in csrc/ derives one of them from the id.  bcBytes: bytes per packed block.  texBytes: bytes per decoded
// block (= the encoder's input block, the measure's source), which also picks the block decode's store: 32 B R11, 64 B 8-bit,
// 128 B BC6H.  mask: the channels measured.  cls: what a texel is.  image: the CVTTMI_PIXELS_* kind of the linear image the
// format decodes into and is measured against (kCvttNoImage: R11 has no image form); an image it is built from has the same
// kind, read as int8 (CVTTMI_PIXELS_RGBA8_SNORM) by the snorm class.  peak: the PSNR peak, 0 = no PSNR (BC6H).
#ifndef CVTTMI_TEXTURE_FORMATS_H
#define CVTTMI_TEXTURE_FORMATS_H
#include <stdint.h>
#include "../../include/cvtt_mi355x.h"

enum CvttTexelClass : uint8_t { kCvttUnorm8, kCvttSnorm8, kCvttHalfRgb, kCvttR11 };
constexpr int8_t kCvttNoImage = -1;
struct CvttTextureFormat
{
    uint8_t bcBytes, texBytes, mask;
    CvttTexelClass cls;
    int8_t image;
    uint16_t peak;
};
static constexpr int kCvttTextureFormatCount = CVTTMI_FMT_COUNT;
static constexpr CvttTextureFormat kCvttTextureFormats[kCvttTextureFormatCount] = {
    {16, 64, 0xf, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},     // BC7
    {8, 64, 0xf, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},      // BC1
    {16, 128, 0x7, kCvttHalfRgb, CVTTMI_PIXELS_RGBA16F, 0},   // BC6HU
    {16, 128, 0x7, kCvttHalfRgb, CVTTMI_PIXELS_RGBA16F, 0},   // BC6HS
    {8, 64, 0x7, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},      // ETC2 RGB
    {16, 64, 0xf, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},     // ETC2 RGBA
    {16, 64, 0xf, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},     // BC2
    {16, 64, 0xf, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},     // BC3
    {8, 64, 0x1, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},      // BC4U
    {8, 64, 0x1, kCvttSnorm8, CVTTMI_PIXELS_RGBA8, 254},      // BC4S
    {16, 64, 0x3, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},     // BC5U
    {16, 64, 0x3, kCvttSnorm8, CVTTMI_PIXELS_RGBA8, 254},     // BC5S
    {8, 64, 0x7, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},      // ETC1
    {8, 64, 0xf, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},      // ETC2 punch-through
    {8, 64, 0x8, kCvttUnorm8, CVTTMI_PIXELS_RGBA8, 255},      // EAC alpha
    {8, 32, 0x1, kCvttR11, kCvttNoImage, 2047},               // R11U
    {8, 32, 0x1, kCvttR11, kCvttNoImage, 2046},               // R11S
};
#endif
