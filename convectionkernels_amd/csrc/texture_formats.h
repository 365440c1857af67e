// Formats of the decode / measure path (include/cvtt_mi355x.h, CVTTMI_FMT_*), shared by the shim and decode_kernel.hip:
// bytes per packed block, bytes per decoded block (= the encoder's input block, the measure's source), channels measured.
#ifndef CVTTMI_TEXTURE_FORMATS_H
#define CVTTMI_TEXTURE_FORMATS_H
#include <stdint.h>

struct CvttTextureFormat
{
    uint8_t bcBytes, texBytes, mask;
};
// BC7, BC1, BC6HU, BC6HS, ETC2 RGB, ETC2 RGBA, BC2, BC3, BC4U, BC4S, BC5U, BC5S, ETC1, ETC2 punch-through, EAC alpha, R11U, R11S
static constexpr int kCvttTextureFormatCount = 17;
static constexpr CvttTextureFormat kCvttTextureFormats[kCvttTextureFormatCount] = {
    {16, 64, 0xf}, {8, 64, 0xf}, {16, 128, 0x7}, {16, 128, 0x7}, {8, 64, 0x7}, {16, 64, 0xf}, {16, 64, 0xf}, {16, 64, 0xf},
    {8, 64, 0x1},  {8, 64, 0x1}, {16, 64, 0x3},  {16, 64, 0x3},  {8, 64, 0x7}, {8, 64, 0xf},  {8, 64, 0x8},  {8, 32, 0x1},
    {8, 32, 0x1}};
#endif
