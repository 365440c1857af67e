"""numpy restatement of the mip filter (include/cvtt_mi355x.h, "mip chains"): the reference of the mip tests.  A helper, not a
test module.  Images are (H, W, 4) arrays: uint8 (RGBA8), int8 (RGBA8 read as SNORM) or uint16 half bit patterns (RGBA16F)."""
import numpy as np


def level_sizes(w, h):
    """[(w_L, h_L)] of the full chain: each max(1, previous >> 1), down to 1x1"""
    sizes = [(w, h)]
    while sizes[-1] != (1, 1):
        sizes.append((max(1, sizes[-1][0] >> 1), max(1, sizes[-1][1] >> 1)))
    return sizes


def downsample(img):
    """one level: the 2x2 box over (2x, 2y), (2x+1, 2y), (2x, 2y+1), (2x+1, 2y+1), coordinates clamped to the last row / column"""
    h, w = img.shape[:2]
    y0, x0 = 2 * np.arange(max(1, h >> 1)), 2 * np.arange(max(1, w >> 1))
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    a, b, c, d = img[y0][:, x0], img[y0][:, x1], img[y1][:, x0], img[y1][:, x1]
    if img.dtype == np.uint16:
        a, b, c, d = (v.view(np.float16).astype(np.float32) for v in (a, b, c, d))
        return (((a + b) + (c + d)) * np.float32(0.25)).astype(np.float16).view(np.uint16)
    a, b, c, d = (v.astype(np.int32) for v in (a, b, c, d))
    return ((a + b + c + d + 2) >> 2).astype(img.dtype)  # >> on int32 is arithmetic: floor((sum + 2) / 4) for int8


def chain(img, levels=None):
    """[level 0 = img, level 1, ...]: every level from the rounded one before it"""
    out = [img]
    for _ in range((len(level_sizes(img.shape[1], img.shape[0])) if levels is None else levels) - 1):
        out.append(downsample(out[-1]))
    return out


def finite_halfs(rng, shape):
    """random finite half bit patterns: every exponent (subnormals, values up to 65504), both signs"""
    bits = rng.integers(0, 1 << 16, shape, dtype=np.uint16)
    bits[(bits & 0x7C00) == 0x7C00] ^= 0x0400  # exponent 31 (inf / NaN) -> 30
    return bits
