"""Compressed texture file -> decoded image on the MI355X: the reverse of packer.py, for the containers it writes.

    python -m convectionkernels_amd.unpacker [-layer N] [-level L | -mips] input.ktx|input.dds output

The container kind comes from the file's magic bytes (KTX 1.1, or DDS with the DX10 header), the format, the size and the mip
levels from the file (container.read_ktx_texture / read_dds_texture).  The blocks are uploaded as the file holds them and decoded
straight into a linear image on the device (Context.decode_image: no padding to groups of eight, no untiling pass).
output: a .npy of the decoded image, (H, W, 4) uint8 -- int8 for bc4s / bc5s, float16 for bc6hu / bc6hs; for the 8-bit
unsigned formats any other extension is written by PIL as an RGBA image.
-layer N: the layer of a texture array or cube file to decode (default 0; a cube's faces are layers 0..5 in the order +X -X +Y -Y
+Z -Z, cube n of a cube array starts at layer 6 n).  A layer is decoded like a file of its own, on views of the file's bytes.
-level L: decode mip level L (default 0) alone.
-mips: decode every level of the file (Context.decode_mips: one launch for the chain) and write each with its number put before
the extension: out.0.npy, out.1.npy, ...
A file marked sRGB (container.colour_space, the packer's -srgb) decodes to the same texels as an unmarked one: the mark tells a
sampler how to read the decoded bytes, the decoder does not convert them.
R11 (r11u / r11s) has no image form and is refused."""
import os
import struct
import sys

import numpy as np

from . import container

USAGE = __doc__.split("\n\n")[1]


def read_layers(path):
    """-> (format name, width, height, layers[layer][level] blocks, cube) of a KTX or DDS file, told apart by the magic bytes"""
    with open(path, "rb") as f:
        raw = f.read()
    if raw[:12] == container._KTX_ID:
        return container.read_ktx_texture(raw)
    if raw[:4] == container._DDS_MAGIC:
        return container.read_dds_texture(raw)
    raise ValueError("%s is neither a KTX 1.1 nor a DDS file" % path)


def read_levels(path, layer=0):
    """-> (format name, width, height, [blocks per level]) of one layer of a KTX or DDS file"""
    fmt, width, height, layers, _ = read_layers(path)
    if layer >= len(layers):
        raise ValueError("%s has %d layer(s), no layer %d" % (path, len(layers), layer))
    return fmt, width, height, layers[layer]


def decode_file_levels(fmt, width, height, levels, ctx=None):
    """the packed levels of a file (numpy, level 0 first) -> [decoded (h_L, w_L, 4) numpy image per level]"""
    import torch
    from . import api
    ctx = ctx or api.default_context()
    packed = torch.from_numpy(np.concatenate([np.ascontiguousarray(l, np.uint8).reshape(-1) for l in levels])).cuda(ctx.device)
    bounds = np.cumsum([0] + [l.size for l in levels])
    images = ctx.decode_mips(fmt, [packed[a:b] for a, b in zip(bounds[:-1], bounds[1:])], width, height)
    torch.cuda.synchronize(ctx.device)
    return [img.cpu().numpy() for img in images]


def decode_file_level(fmt, width, height, packed, ctx=None):
    """the packed blocks of one width x height image (numpy) -> its decoded (H, W, 4) numpy image"""
    import torch
    from . import api
    ctx = ctx or api.default_context()
    image = ctx.decode_image(fmt, torch.from_numpy(np.ascontiguousarray(packed, np.uint8)).cuda(ctx.device), width, height)
    torch.cuda.synchronize(ctx.device)
    return image.cpu().numpy()


def write_image(path, image):
    if path.endswith(".npy"):
        np.save(path, image)
    elif image.dtype != np.uint8:
        raise ValueError("%s: a %s image is written as .npy only" % (path, image.dtype))
    else:
        from PIL import Image  # only needed for image files
        Image.fromarray(image, "RGBA").save(path)


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    level, mips, layer, paths = None, False, 0, []
    i = 0
    while i < len(argv):
        a = argv[i]
        if a == "-level" and i + 1 < len(argv) and argv[i + 1].isdigit():
            level = int(argv[i + 1])
            i += 1
        elif a == "-layer" and i + 1 < len(argv) and argv[i + 1].isdigit():
            layer = int(argv[i + 1])
            i += 1
        elif a == "-mips":
            mips = True
        elif a.startswith("-"):
            sys.stderr.write(USAGE + "\n")
            return 2
        else:
            paths.append(a)
        i += 1
    if len(paths) != 2 or (mips and level is not None):
        sys.stderr.write(USAGE + "\n")
        return 2
    try:
        fmt, width, height, levels = read_levels(paths[0], layer)
        if fmt in ("r11u", "r11s"):
            raise ValueError("%s: %s has no image form" % (paths[0], fmt))
        if (level or 0) >= len(levels):
            raise ValueError("%s has %d mip level(s), no level %d" % (paths[0], len(levels), level))
        stem, ext = os.path.splitext(paths[1])
        if ext != ".npy" and fmt in ("bc4s", "bc5s", "bc6hu", "bc6hs"):
            raise ValueError("%s decodes to %s: the output must be a .npy" % (fmt, "float16" if fmt.startswith("bc6") else "int8"))
    except (ValueError, OSError, struct.error) as e:
        sys.stderr.write("%s\n" % e)
        return 1
    try:
        if mips:
            for l, image in enumerate(decode_file_levels(fmt, width, height, levels)):
                write_image("%s.%d%s" % (stem, l, ext), image)
        else:
            w, h = container.mip_sizes(width, height, len(levels))[level or 0]
            write_image(paths[1], decode_file_level(fmt, w, h, levels[level or 0]))
    except (ValueError, OSError) as e:  # (a CvttError is a failure of the device path, not of the command line: it propagates)
        sys.stderr.write("%s\n" % e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
