"""Decoded blocks -> the linear image they tile (test helper, plain numpy): the inverse of texture_decode_ref.image_to_blocks
on the texels inside the image."""
import numpy as np


def untile(blocks, width, height):
    """(bw * bh, 16, C) decoded blocks, row-major with bw = ceil(width / 4) blocks per row, texel p = 4 * row + column
    -> the (height, width, C) image; the texels of the edge blocks beyond width x height are dropped"""
    bw, bh = (width + 3) // 4, (height + 3) // 4
    b = np.asarray(blocks)
    assert b.ndim == 3 and b.shape[:2] == (bw * bh, 16), (b.shape, width, height)
    full = b.reshape(bh, bw, 4, 4, b.shape[2]).transpose(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, b.shape[2])
    return np.ascontiguousarray(full[:height, :width])
