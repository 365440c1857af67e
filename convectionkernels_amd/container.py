"""Texture containers for the packed blocks ("container writer").

The encoders return blocks row-major, ceil(W/4) per row -- exactly the payload order of a KTX 1.1 mip level and of a
DDS surface, so a container is a header in front of the device output.  KTX mirrors what the reference's example
packer writes (etc2packer.cpp:116-197: one level, one face, no key/value data, little endian); DDS (DX10 header) is
added for the BC formats.  `read_ktx` / `read_dds` exist for the tests and for tools that want the blocks back."""
import struct

import numpy as np

# name -> (bytes per block, GL internal format, GL base internal format, DXGI format or None)
_GL_RGB, _GL_RGBA, _GL_RED, _GL_RG = 0x1907, 0x1908, 0x1903, 0x8227
FORMATS = {
    "etc1": (8, 0x8D64, _GL_RGB, None),             # GL_ETC1_RGB8_OES
    "etc2": (8, 0x9274, _GL_RGB, None),             # GL_COMPRESSED_RGB8_ETC2
    "etc2rgba": (16, 0x9278, _GL_RGBA, None),       # GL_COMPRESSED_RGBA8_ETC2_EAC
    "etc2punchthrough": (8, 0x9276, _GL_RGBA, None),  # GL_COMPRESSED_RGB8_PUNCHTHROUGH_ALPHA1_ETC2
    "r11u": (8, 0x9270, _GL_RED, None),             # GL_COMPRESSED_R11_EAC
    "r11s": (8, 0x9271, _GL_RED, None),             # GL_COMPRESSED_SIGNED_R11_EAC
    "bc1": (8, 0x83F1, _GL_RGBA, 71),               # GL_COMPRESSED_RGBA_S3TC_DXT1_EXT / DXGI_FORMAT_BC1_UNORM
    "bc2": (16, 0x83F2, _GL_RGBA, 74),
    "bc3": (16, 0x83F3, _GL_RGBA, 77),
    "bc4u": (8, 0x8DBB, _GL_RED, 80),               # GL_COMPRESSED_RED_RGTC1
    "bc4s": (8, 0x8DBC, _GL_RED, 81),
    "bc5u": (16, 0x8DBD, _GL_RG, 83),
    "bc5s": (16, 0x8DBE, _GL_RG, 84),
    "bc6hu": (16, 0x8E8F, _GL_RGB, 95),             # GL_COMPRESSED_RGB_BPTC_UNSIGNED_FLOAT
    "bc6hs": (16, 0x8E8E, _GL_RGB, 96),
    "bc7": (16, 0x8E8C, _GL_RGBA, 98),              # GL_COMPRESSED_RGBA_BPTC_UNORM
}
# name -> (GL internal format, DXGI format or None) of the format's sRGB form: what `srgb=True` writes.  The readers take both
# codes and return the same name; colour_space tells them apart.  Formats not listed here have no sRGB code.
SRGB_FORMATS = {
    "etc2": (0x9275, None),              # GL_COMPRESSED_SRGB8_ETC2
    "etc2punchthrough": (0x9277, None),  # GL_COMPRESSED_SRGB8_PUNCHTHROUGH_ALPHA1_ETC2
    "etc2rgba": (0x9279, None),          # GL_COMPRESSED_SRGB8_ALPHA8_ETC2_EAC
    "bc1": (0x8C4D, 72),                 # GL_COMPRESSED_SRGB_ALPHA_S3TC_DXT1_EXT / DXGI_FORMAT_BC1_UNORM_SRGB
    "bc2": (0x8C4E, 75),
    "bc3": (0x8C4F, 78),
    "bc7": (0x8E8D, 99),                 # GL_COMPRESSED_SRGB_ALPHA_BPTC_UNORM
}
# the names the reference's packer uses on its command line (etc2packer.cpp:34-42)
ALIASES = {"etc2rgb": "etc2"}

_KTX_ID = bytes([0xAB, 0x4B, 0x54, 0x58, 0x20, 0x31, 0x31, 0xBB, 0x0D, 0x0A, 0x1A, 0x0A])
_DDS_MAGIC = b"DDS "


def canonical(fmt):
    fmt = ALIASES.get(fmt, fmt)
    if fmt not in FORMATS:
        raise ValueError("unknown texture format %r" % (fmt,))
    return fmt


def _codes(fmt, srgb):
    """(GL internal format, DXGI format or None) to write for a canonical format name"""
    if not srgb:
        return FORMATS[fmt][1], FORMATS[fmt][3]
    if fmt not in SRGB_FORMATS:
        raise ValueError("%s has no sRGB format code" % fmt)
    return SRGB_FORMATS[fmt]


def _gl_names(internal):
    return [n for n, v in FORMATS.items() if v[1] == internal] or [n for n, v in SRGB_FORMATS.items() if v[0] == internal]


def _dxgi_names(dxgi):
    return [n for n, v in FORMATS.items() if v[3] == dxgi] or [n for n, v in SRGB_FORMATS.items() if v[1] == dxgi]


def colour_space(path_or_bytes):
    """"srgb" if a KTX or DDS file carries the sRGB code of its format (written with srgb=True), "linear" otherwise"""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if raw[:12] == _KTX_ID:
        internal = struct.unpack_from("<13I", raw, 12)[4]
        if not _gl_names(internal):
            raise ValueError("unsupported glInternalFormat 0x%x" % internal)
        return "srgb" if any(v[0] == internal for v in SRGB_FORMATS.values()) else "linear"
    if raw[:4] == _DDS_MAGIC and raw[84:88] == b"DX10":
        dxgi, = struct.unpack_from("<I", raw, 128)
        if not _dxgi_names(dxgi):
            raise ValueError("unsupported DXGI format %d" % dxgi)
        return "srgb" if any(v[1] == dxgi for v in SRGB_FORMATS.values()) else "linear"
    raise ValueError("neither a KTX 1.1 nor a DX10 DDS file")


def _payload(fmt, width, height, packed):
    per = FORMATS[fmt][0]
    bw, bh = (width + 3) // 4, (height + 3) // 4
    if hasattr(packed, "detach"):  # torch tensor (device or host)
        packed = packed.detach().cpu().numpy()
    data = np.ascontiguousarray(packed, dtype=np.uint8).reshape(-1)
    if data.size != bw * bh * per:
        raise ValueError("%s %dx%d needs %d bytes of blocks, got %d" % (fmt, width, height, bw * bh * per, data.size))
    return data


def ktx_bytes(fmt, width, height, packed, srgb=False):
    """KTX 1.1 file image: the 64-byte header of etc2packer.cpp:123-147, imageSize, blocks.  srgb: write the format's sRGB
    code (SRGB_FORMATS; ValueError for a format without one) -- a mark for the sampler, the blocks are the same."""
    fmt = canonical(fmt)
    internal, base = _codes(fmt, srgb)[0], FORMATS[fmt][2]
    data = _payload(fmt, width, height, packed)
    header = _KTX_ID + struct.pack("<13I", 0x04030201, 0, 1, 0, internal, base, width, height, 0, 0, 1, 1, 0)
    return header + struct.pack("<I", data.size) + data.tobytes()


def write_ktx(path, fmt, width, height, packed, srgb=False):
    with open(path, "wb") as f:
        f.write(ktx_bytes(fmt, width, height, packed, srgb))


def read_ktx(path_or_bytes):
    """-> (format name, width, height, blocks (N, bytesPerBlock) uint8)"""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if raw[:12] != _KTX_ID:
        raise ValueError("not a KTX 1.1 file")
    f = struct.unpack_from("<13I", raw, 12)
    if f[0] != 0x04030201:
        raise ValueError("big-endian KTX is not supported")
    internal, width, height, kv = f[4], f[6], f[7], f[12]
    names = _gl_names(internal)
    if not names:
        raise ValueError("unsupported glInternalFormat 0x%x" % internal)
    off = 64 + kv
    size, = struct.unpack_from("<I", raw, off)
    per = FORMATS[names[0]][0]
    blocks = np.frombuffer(raw, np.uint8, size, off + 4).reshape(-1, per).copy()
    return names[0], width, height, blocks


def dds_bytes(fmt, width, height, packed, srgb=False):
    """DDS with the DX10 extension header (BC formats only): one 2-D surface, one mip level.  srgb: as for ktx_bytes."""
    fmt = canonical(fmt)
    if FORMATS[fmt][3] is None:
        raise ValueError("%s has no DXGI format; use KTX" % fmt)
    dxgi = _codes(fmt, srgb)[1]
    data = _payload(fmt, width, height, packed)
    DDSD_CAPS, DDSD_HEIGHT, DDSD_WIDTH, DDSD_PIXELFORMAT, DDSD_LINEARSIZE = 0x1, 0x2, 0x4, 0x1000, 0x80000
    flags = DDSD_CAPS | DDSD_HEIGHT | DDSD_WIDTH | DDSD_PIXELFORMAT | DDSD_LINEARSIZE
    pixel_format = struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)  # DDPF_FOURCC
    header = struct.pack("<7I", 124, flags, height, width, data.size, 0, 1) + bytes(44) + pixel_format + \
        struct.pack("<5I", 0x1000, 0, 0, 0, 0)  # DDSCAPS_TEXTURE
    assert len(header) == 124
    dx10 = struct.pack("<5I", dxgi, 3, 0, 1, 0)  # D3D10_RESOURCE_DIMENSION_TEXTURE2D, array size 1
    return _DDS_MAGIC + header + dx10 + data.tobytes()


def write_dds(path, fmt, width, height, packed, srgb=False):
    with open(path, "wb") as f:
        f.write(dds_bytes(fmt, width, height, packed, srgb))


def read_dds(path_or_bytes):
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if raw[:4] != _DDS_MAGIC or raw[84:88] != b"DX10":
        raise ValueError("not a DX10 DDS file")
    height, width = struct.unpack_from("<2I", raw, 12)
    dxgi, = struct.unpack_from("<I", raw, 128)
    names = _dxgi_names(dxgi)
    if not names:
        raise ValueError("unsupported DXGI format %d" % dxgi)
    per = FORMATS[names[0]][0]
    n = ((width + 3) // 4) * ((height + 3) // 4)
    blocks = np.frombuffer(raw, np.uint8, n * per, 148).reshape(n, per).copy()
    return names[0], width, height, blocks


# ---- mip chains: level 0 first in both containers, so read_ktx / read_dds above return level 0 of these files ----

def mip_sizes(width, height, levels):
    """[(w_L, h_L)] of the first `levels` levels: each max(1, previous >> 1); at most floor(log2(max(w, h))) + 1 of them"""
    full = max(int(width), int(height), 1).bit_length()
    if width < 1 or height < 1 or not 1 <= levels <= full:
        raise ValueError("a %dx%d texture has 1 .. %d mip levels, got %d" % (width, height, full, levels))
    return [(max(1, width >> l), max(1, height >> l)) for l in range(levels)]


def _mip_payloads(fmt, width, height, levels):
    levels = list(levels)
    return [_payload(fmt, w, h, packed) for (w, h), packed in zip(mip_sizes(width, height, len(levels)), levels)]


def ktx_mips_bytes(fmt, width, height, levels, srgb=False):
    """KTX 1.1 with numberOfMipmapLevels = len(levels): per level a uint32 imageSize and its blocks (what
    Context.encode_mips returns, level 0 first).  Blocks are 8 or 16 bytes, so the mip padding to 4 bytes is always empty.
    srgb: as for ktx_bytes."""
    fmt = canonical(fmt)
    internal, base = _codes(fmt, srgb)[0], FORMATS[fmt][2]
    data = _mip_payloads(fmt, width, height, levels)
    header = _KTX_ID + struct.pack("<13I", 0x04030201, 0, 1, 0, internal, base, width, height, 0, 0, 1, len(data), 0)
    return header + b"".join(struct.pack("<I", d.size) + d.tobytes() for d in data)


def write_ktx_mips(path, fmt, width, height, levels, srgb=False):
    with open(path, "wb") as f:
        f.write(ktx_mips_bytes(fmt, width, height, levels, srgb))


def read_ktx_mips(path_or_bytes):
    """-> (format name, width, height, [blocks (N_L, bytesPerBlock) uint8 per level])"""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    name, width, height, _ = read_ktx(raw)
    count, kv = struct.unpack_from("<2I", raw, 12 + 4 * 11)
    per = FORMATS[name][0]
    off, levels = 64 + kv, []
    for w, h in mip_sizes(width, height, max(1, count)):
        size, = struct.unpack_from("<I", raw, off)
        if size != ((w + 3) // 4) * ((h + 3) // 4) * per:
            raise ValueError("mip level %d (%dx%d) holds %d bytes" % (len(levels), w, h, size))
        levels.append(np.frombuffer(raw, np.uint8, size, off + 4).reshape(-1, per).copy())
        off += 4 + (size + 3) // 4 * 4
    return name, width, height, levels


def dds_mips_bytes(fmt, width, height, levels, srgb=False):
    """DDS (DX10 header) with dwMipMapCount = len(levels): the levels' blocks one after the other behind the headers.  More
    than one level sets DDSD_MIPMAPCOUNT and DDSCAPS_COMPLEX | DDSCAPS_MIPMAP; pitchOrLinearSize is level 0's size.
    srgb: as for ktx_bytes."""
    fmt = canonical(fmt)
    if FORMATS[fmt][3] is None:
        raise ValueError("%s has no DXGI format; use KTX" % fmt)
    dxgi = _codes(fmt, srgb)[1]
    data = _mip_payloads(fmt, width, height, levels)
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000  # DDSD_CAPS | HEIGHT | WIDTH | PIXELFORMAT | LINEARSIZE
    caps = 0x1000  # DDSCAPS_TEXTURE
    if len(data) > 1:
        flags |= 0x20000  # DDSD_MIPMAPCOUNT
        caps |= 0x8 | 0x400000  # DDSCAPS_COMPLEX | DDSCAPS_MIPMAP
    pixel_format = struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)  # DDPF_FOURCC
    header = struct.pack("<7I", 124, flags, height, width, data[0].size, 0, len(data)) + bytes(44) + pixel_format + \
        struct.pack("<5I", caps, 0, 0, 0, 0)
    dx10 = struct.pack("<5I", dxgi, 3, 0, 1, 0)  # D3D10_RESOURCE_DIMENSION_TEXTURE2D, array size 1
    return _DDS_MAGIC + header + dx10 + b"".join(d.tobytes() for d in data)


def write_dds_mips(path, fmt, width, height, levels, srgb=False):
    with open(path, "wb") as f:
        f.write(dds_mips_bytes(fmt, width, height, levels, srgb))


def read_dds_mips(path_or_bytes):
    """-> (format name, width, height, [blocks per level]); a file without DDSD_MIPMAPCOUNT has one level"""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    name, width, height, _ = read_dds(raw)
    flags, = struct.unpack_from("<I", raw, 8)
    count, = struct.unpack_from("<I", raw, 28)
    per = FORMATS[name][0]
    off, levels = 148, []
    for w, h in mip_sizes(width, height, max(1, count) if flags & 0x20000 else 1):
        n = ((w + 3) // 4) * ((h + 3) // 4)
        if off + n * per > len(raw):
            raise ValueError("mip level %d (%dx%d) is cut short" % (len(levels), w, h))
        levels.append(np.frombuffer(raw, np.uint8, n * per, off).reshape(n, per).copy())
        off += n * per
    return name, width, height, levels


# ---- texture arrays and cube maps: `layers` = [layer][level] packed blocks (what Context.encode_texture returns), layer =
# array element x faces + face, the faces of a cube in the order +X -X +Y -Y +Z -Z.  KTX stores level-major (every level's
# layers consecutive), DDS layer-major (every layer's chain consecutive): encode_texture's order="level" / "layer". ----

def _texture_payloads(fmt, width, height, layers, cube):
    """[layer][level] -> the same as checked uint8 byte arrays.  ValueError: no layers, a cube that is not square or whose layers
    are no multiple of 6, layers of unequal level counts, a wrong block count in any (layer, level)."""
    base = getattr(layers, "base", None)
    layers = [list(levels) for levels in layers]
    if not layers:
        raise ValueError("a texture has at least one layer")
    if cube and (width != height or len(layers) % 6 != 0):
        raise ValueError("a cube needs square faces and 6 n layers, got %dx%d and %d layer(s)" % (width, height, len(layers)))
    if any(len(levels) != len(layers[0]) for levels in layers):
        raise ValueError("every layer needs the same number of mip levels, got %s" % sorted({len(levels) for levels in layers}))
    if base is not None and hasattr(base, "data_ptr"):
        # the views of one device allocation: one copy to the host, the same views of that copy
        host, start, per = base.detach().cpu().numpy().reshape(-1), base.data_ptr(), FORMATS[fmt][0]
        layers = [[host[t.data_ptr() - start: t.data_ptr() - start + t.shape[0] * per] for t in levels] for levels in layers]
    return [_mip_payloads(fmt, width, height, levels) for levels in layers]


def ktx_texture_bytes(fmt, width, height, layers, cube=False, srgb=False):
    """KTX 1.1 of a 2-D texture, a texture array, a cube or a cube array.  numberOfFaces = 6 for cubes, else 1;
    numberOfArrayElements = 0 for a single texture or a single cube, else the element count (cubes, for a cube array).  Per level
    one uint32 imageSize, then the level of every element, inside an element of every face.  imageSize is the bytes of ONE FACE for
    a non-array cube (KTX 1 specification, 2.16) and of the whole level in every other case.  Blocks are 8 or 16 bytes, so cube and
    mip padding are always empty.  One layer, not a cube: the bytes of ktx_mips_bytes.  srgb: as for ktx_bytes."""
    fmt = canonical(fmt)
    internal, base = _codes(fmt, srgb)[0], FORMATS[fmt][2]
    data = _texture_payloads(fmt, width, height, layers, cube)
    faces = 6 if cube else 1
    elements = len(data) // faces
    header = _KTX_ID + struct.pack("<13I", 0x04030201, 0, 1, 0, internal, base, width, height, 0, 0 if elements == 1 else elements, faces,
                                   len(data[0]), 0)
    out = [header]
    for level in range(len(data[0])):
        one = data[0][level].size
        out.append(struct.pack("<I", one if cube and elements == 1 else one * len(data)))
        out.extend(d[level].tobytes() for d in data)
    return b"".join(out)


def write_ktx_texture(path, fmt, width, height, layers, cube=False, srgb=False):
    with open(path, "wb") as f:
        f.write(ktx_texture_bytes(fmt, width, height, layers, cube, srgb))


def read_ktx_texture(path_or_bytes):
    """-> (format name, width, height, layers[layer][level] blocks (N, bytesPerBlock) uint8, cube); every file ktx_bytes and
    ktx_mips_bytes write reads as one layer"""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    name, width, height, _ = read_ktx(raw)
    elements, faces, count, kv = struct.unpack_from("<4I", raw, 12 + 4 * 9)
    if faces not in (1, 6):
        raise ValueError("numberOfFaces is %d" % faces)
    cube = faces == 6
    n = max(1, elements) * faces
    per = FORMATS[name][0]
    off, layers = 64 + kv, [[] for _ in range(n)]
    for level, (w, h) in enumerate(mip_sizes(width, height, max(1, count))):
        size, = struct.unpack_from("<I", raw, off)
        one = ((w + 3) // 4) * ((h + 3) // 4) * per
        if size != (one if cube and elements == 0 else one * n):
            raise ValueError("mip level %d (%dx%d, %d layer(s)) holds %d bytes" % (level, w, h, n, size))
        off += 4
        if off + one * n > len(raw):
            raise ValueError("mip level %d (%dx%d) is cut short" % (level, w, h))
        for layer in range(n):
            layers[layer].append(np.frombuffer(raw, np.uint8, one, off).reshape(-1, per).copy())
            off += one
    return name, width, height, layers, cube


def dds_texture_bytes(fmt, width, height, layers, cube=False, srgb=False):
    """DDS (DX10 header) of a 2-D texture, a texture array, a cube or a cube array: arraySize = the elements (cubes, for a cube
    file), miscFlag = 0x4 (DDS_RESOURCE_MISC_TEXTURECUBE) for cubes, which also set DDSCAPS_COMPLEX and dwCaps2 = DDSCAPS2_CUBEMAP
    with all six face bits (0xFE00).  The payload is layer-major: every layer's chain, level 0 first; the mip fields are those of
    dds_mips_bytes.  One layer, not a cube: the bytes of dds_mips_bytes.  srgb: as for ktx_bytes."""
    fmt = canonical(fmt)
    if FORMATS[fmt][3] is None:
        raise ValueError("%s has no DXGI format; use KTX" % fmt)
    dxgi = _codes(fmt, srgb)[1]
    data = _texture_payloads(fmt, width, height, layers, cube)
    flags = 0x1 | 0x2 | 0x4 | 0x1000 | 0x80000  # DDSD_CAPS | HEIGHT | WIDTH | PIXELFORMAT | LINEARSIZE
    caps, caps2 = 0x1000, 0  # DDSCAPS_TEXTURE
    if len(data[0]) > 1:
        flags |= 0x20000  # DDSD_MIPMAPCOUNT
        caps |= 0x8 | 0x400000  # DDSCAPS_COMPLEX | DDSCAPS_MIPMAP
    if cube:
        caps |= 0x8
        caps2 = 0xFE00  # DDSCAPS2_CUBEMAP | the six DDSCAPS2_CUBEMAP_*
    pixel_format = struct.pack("<2I4s5I", 32, 0x4, b"DX10", 0, 0, 0, 0, 0)  # DDPF_FOURCC
    header = struct.pack("<7I", 124, flags, height, width, data[0][0].size, 0, len(data[0])) + bytes(44) + pixel_format + \
        struct.pack("<5I", caps, caps2, 0, 0, 0)
    dx10 = struct.pack("<5I", dxgi, 3, 0x4 if cube else 0, len(data) // (6 if cube else 1), 0)  # D3D10_RESOURCE_DIMENSION_TEXTURE2D
    return _DDS_MAGIC + header + dx10 + b"".join(d.tobytes() for levels in data for d in levels)


def write_dds_texture(path, fmt, width, height, layers, cube=False, srgb=False):
    with open(path, "wb") as f:
        f.write(dds_texture_bytes(fmt, width, height, layers, cube, srgb))


def read_dds_texture(path_or_bytes):
    """-> (format name, width, height, layers[layer][level] blocks, cube); every file dds_bytes and dds_mips_bytes write reads as
    one layer"""
    raw = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    name, width, height, _ = read_dds(raw)
    flags, = struct.unpack_from("<I", raw, 8)
    count, = struct.unpack_from("<I", raw, 28)
    misc, elements = struct.unpack_from("<2I", raw, 136)
    cube = bool(misc & 0x4)
    n = max(1, elements) * (6 if cube else 1)
    per = FORMATS[name][0]
    off, layers = 148, []
    sizes = mip_sizes(width, height, max(1, count) if flags & 0x20000 else 1)
    for layer in range(n):
        levels = []
        for level, (w, h) in enumerate(sizes):
            blocks = ((w + 3) // 4) * ((h + 3) // 4)
            if off + blocks * per > len(raw):
                raise ValueError("layer %d, mip level %d (%dx%d) is cut short" % (layer, level, w, h))
            levels.append(np.frombuffer(raw, np.uint8, blocks * per, off).reshape(blocks, per).copy())
            off += blocks * per
        layers.append(levels)
    return name, width, height, layers, cube
