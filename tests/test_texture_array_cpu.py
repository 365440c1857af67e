"""Texture arrays and cube maps without a device: cvttmi_texture_layout / cvttmi_texture_subresource against a restatement of
the header's two formulas over api.mip_layout, the KTX / DDS writers and readers for arrays and cubes field by field, and the
packer's argument errors."""
import struct

import numpy as np
import pytest

from convectionkernels_amd import api, container, packer

SIZES = [(1, 1), (5, 70), (37, 21), (32, 32), (260, 9), (4096, 4096)]
LAYERS = [1, 2, 6, 12]


def _expected_place(table, order, layers, layer, level):
    """the header's formulas: T = cvttmi_mip_layout's table, E = T[levels].firstBlock"""
    T, E = table, table.block_count
    if order == "layer":
        return layer * E + T[level].firstBlock, T[level].blockCount
    return layers * T[level].firstBlock + layer * T[level].blockCount, T[level].blockCount


@pytest.mark.parametrize("width,height", SIZES)
@pytest.mark.parametrize("bpb,pixel_bytes", [(8, 4), (16, 4), (16, 8)])
def test_layout_and_subresources(width, height, bpb, pixel_bytes):
    full = api.mip_level_count(width, height)
    for levels in sorted({1, min(2, full), full}):
        T = api.mip_layout(width, height, pixel_bytes, bpb, levels)
        for layers in LAYERS:
            for order in ("layer", "level"):
                s = api.texture_layout(width, height, pixel_bytes, bpb, levels, layers, order)
                per_layer = (T.pyramid_bytes + 255) // 256 * 256
                assert (s.pyramidLayerBytes, s.pyramidBytes) == (per_layer, per_layer * layers)
                assert (s.tilesPerLayer, s.tiles) == (T.tile_count, T.tile_count * layers)
                assert (s.blocksPerLayer, s.blocks) == (T.block_count, T.block_count * layers)
                # pyramids, tiles (16 texels each) and padded packed blocks all fit
                assert s.workBytes >= s.pyramidBytes + s.tiles * 16 * pixel_bytes + s.tiles * bpb
                places = []
                for layer in range(layers):
                    for level in range(levels):
                        got = api.texture_subresource(width, height, pixel_bytes, bpb, levels, layers, order, layer, level)
                        assert got == _expected_place(T, order, layers, layer, level), (order, layers, layer, level)
                        places.append(got)
                # the subresources tile [0, blocks) without gap or overlap
                at = 0
                for first, count in sorted(places):
                    assert first == at and count > 0
                    at += count
                assert at == s.blocks


def test_layout_levels_default_is_the_full_chain():
    assert api.texture_layout(37, 21, 4, 16, None, 3).blocks == api.texture_layout(37, 21, 4, 16, 6, 3).blocks
    assert api.texture_subresource(37, 21, 4, 16, None, 3, "level", 2, 5) == api.texture_subresource(37, 21, 4, 16, 6, 3, "level", 2, 5)


def test_layout_rejections():
    ok = dict(width=37, height=21, pixel_bytes=4, bytes_per_block=16, levels=3, layers=2, order="layer")
    api.texture_layout(**ok)
    for change in (dict(layers=0), dict(width=0), dict(height=0), dict(pixel_bytes=3), dict(bytes_per_block=4), dict(levels=0), dict(levels=7),
                   dict(order=2), dict(order=-1)):
        with pytest.raises(api.CvttError):
            api.texture_layout(**dict(ok, **change))
    with pytest.raises(api.CvttError):
        api.texture_layout(**dict(ok, order="face"))
    # 2^32 or more tiles / blocks in total: 4096^2 has 2^20 blocks at level 0
    api.texture_layout(4096, 4096, 4, 16, 1, 4095)
    with pytest.raises(api.CvttError):
        api.texture_layout(4096, 4096, 4, 16, 1, 4096)
    # 8 x 4 has one group of 8 tiles but 2 blocks: the tiles alone reach 2^32
    api.texture_layout(8, 4, 4, 8, 1, (1 << 29) - 1)
    with pytest.raises(api.CvttError):
        api.texture_layout(8, 4, 4, 8, 1, 1 << 29)
    # sizes beyond size_t: the largest image's pyramid fits once, not 2^32 - 1 times
    big = 0xFFFFFFFF
    with pytest.raises(api.CvttError):
        api.texture_layout(big, big, 8, 16, 2, big)
    api.mip_layout(1 << 31, 1 << 31, 4, 16, 2)  # one layer's 2^62-byte pyramid is a size_t ...
    with pytest.raises(api.CvttError):
        api.texture_layout(1 << 31, 1 << 31, 4, 16, 2, 4)  # ... four of them are not
    for change in (dict(layer=2), dict(level=3)):
        with pytest.raises(api.CvttError):
            api.texture_subresource(**dict(dict(ok, layer=0, level=0), **change))
    # nothing is written on failure
    lib = api.load_library()
    out = api.TextureSizes()
    import ctypes
    ctypes.memset(ctypes.addressof(out), 0xAB, ctypes.sizeof(out))
    assert lib.cvttmi_texture_layout(37, 21, api.PIXELS_RGBA8, 16, 3, 0, 0, ctypes.byref(out)) == -1
    assert bytes(out) == b"\xAB" * ctypes.sizeof(out)
    assert lib.cvttmi_texture_layout(37, 21, api.PIXELS_RGBA8, 16, 3, 2, 0, None) == -1
    first, count = ctypes.c_size_t(77), ctypes.c_size_t(78)
    assert lib.cvttmi_texture_subresource(37, 21, api.PIXELS_RGBA8, 16, 3, 2, 0, 2, 0, ctypes.byref(first), ctypes.byref(count)) == -1
    assert (first.value, count.value) == (77, 78)


# ---- containers ----

def _texture(fmt, width, height, layers, levels, seed=5):
    """[layer][level] random blocks of the right counts"""
    per = container.FORMATS[fmt][0]
    rng = np.random.default_rng(seed)
    return [[rng.integers(0, 256, (((w + 3) // 4) * ((h + 3) // 4), per), dtype=np.uint8) for w, h in container.mip_sizes(width, height, levels)]
            for _ in range(layers)]


def _same(a, b):
    assert len(a) == len(b)
    for la, lb in zip(a, b):
        assert len(la) == len(lb)
        for x, y in zip(la, lb):
            assert x.shape == y.shape and (x == y).all()


@pytest.mark.parametrize("levels", [1, 6])
def test_one_layer_is_the_mips_file(levels):
    tex = _texture("bc7", 37, 21, 1, levels)
    for srgb in (False, True):
        assert container.ktx_texture_bytes("bc7", 37, 21, tex, srgb=srgb) == container.ktx_mips_bytes("bc7", 37, 21, tex[0], srgb=srgb)
        assert container.dds_texture_bytes("bc7", 37, 21, tex, srgb=srgb) == container.dds_mips_bytes("bc7", 37, 21, tex[0], srgb=srgb)
    tex = _texture("etc2", 37, 21, 1, levels)
    assert container.ktx_texture_bytes("etc2rgb", 37, 21, tex) == container.ktx_mips_bytes("etc2", 37, 21, tex[0])


CASES = [("cube", 6, True), ("array3", 3, False), ("cubes2", 12, True)]


@pytest.mark.parametrize("name,layers,cube", CASES)
@pytest.mark.parametrize("levels", [1, 6])
@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_ktx_fields_and_round_trip(name, layers, cube, levels, fmt):
    size = 32
    per = container.FORMATS[fmt][0]
    tex = _texture(fmt, size, size, layers, levels)
    raw = container.ktx_texture_bytes(fmt, size, size, tex, cube=cube)
    f = struct.unpack_from("<13I", raw, 12)
    elements = layers // 6 if cube else layers
    assert f[0] == 0x04030201 and f[4] == container.FORMATS[fmt][1]
    assert (f[6], f[7], f[8]) == (size, size, 0)
    assert f[9] == (0 if elements == 1 else elements)   # numberOfArrayElements
    assert f[10] == (6 if cube else 1)                   # numberOfFaces
    assert f[11] == levels and f[12] == 0
    # the payload: per level one imageSize, then element by element, face by face = layer by layer
    off = 64
    for level, (w, h) in enumerate(container.mip_sizes(size, size, levels)):
        one = ((w + 3) // 4) * ((h + 3) // 4) * per
        image_size, = struct.unpack_from("<I", raw, off)
        assert image_size == (one if name == "cube" else one * layers), (name, level)  # one FACE for a non-array cube
        off += 4
        for layer in range(layers):
            assert raw[off: off + one] == tex[layer][level].tobytes(), (layer, level)
            off += one
    assert off == len(raw)
    got = container.read_ktx_texture(raw)
    assert got[:3] == (fmt, size, size) and got[4] is cube
    _same(got[3], tex)


@pytest.mark.parametrize("name,layers,cube", CASES)
@pytest.mark.parametrize("levels", [1, 6])
@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_dds_fields_and_round_trip(name, layers, cube, levels, fmt):
    size = 32
    tex = _texture(fmt, size, size, layers, levels)
    raw = container.dds_texture_bytes(fmt, size, size, tex, cube=cube)
    assert raw[:4] == b"DDS " and raw[84:88] == b"DX10"
    flags, height, width, linear, _, mips = struct.unpack_from("<6I", raw, 8)
    caps, caps2 = struct.unpack_from("<2I", raw, 108)
    dxgi, dim, misc, array_size, _ = struct.unpack_from("<5I", raw, 128)
    assert (height, width, linear, mips) == (size, size, tex[0][0].size, levels)
    assert bool(flags & 0x20000) == (levels > 1)                       # DDSD_MIPMAPCOUNT
    assert bool(caps & 0x400000) == (levels > 1) and caps & 0x1000     # DDSCAPS_MIPMAP, DDSCAPS_TEXTURE
    assert bool(caps & 0x8) == (levels > 1 or cube)                    # DDSCAPS_COMPLEX
    assert caps2 == (0xFE00 if cube else 0)                            # DDSCAPS2_CUBEMAP | all six faces
    assert dxgi == container.FORMATS[fmt][3] and dim == 3
    assert misc == (0x4 if cube else 0)                                # DDS_RESOURCE_MISC_TEXTURECUBE
    assert array_size == (layers // 6 if cube else layers)
    assert raw[148:] == b"".join(level.tobytes() for chain in tex for level in chain)  # layer-major
    got = container.read_dds_texture(raw)
    assert got[:3] == (fmt, size, size) and got[4] is cube
    _same(got[3], tex)


def test_readers_take_the_existing_writers_files():
    tex = _texture("bc3", 37, 21, 1, 6)
    for read, raws in ((container.read_ktx_texture, (container.ktx_bytes("bc3", 37, 21, tex[0][0]), container.ktx_mips_bytes("bc3", 37, 21, tex[0]))),
                       (container.read_dds_texture, (container.dds_bytes("bc3", 37, 21, tex[0][0]), container.dds_mips_bytes("bc3", 37, 21, tex[0])))):
        for raw, levels in zip(raws, (1, 6)):
            fmt, w, h, layers, cube = read(raw)
            assert (fmt, w, h, cube) == ("bc3", 37, 21, False)
            _same(layers, [tex[0][:levels]])


@pytest.mark.parametrize("write", [container.ktx_texture_bytes, container.dds_texture_bytes])
def test_container_errors(write):
    with pytest.raises(ValueError):
        write("bc7", 32, 16, _texture("bc7", 32, 16, 6, 1), cube=True)      # a cube that is not square
    with pytest.raises(ValueError):
        write("bc7", 32, 32, _texture("bc7", 32, 32, 7, 1), cube=True)      # 7 cube layers
    tex = _texture("bc7", 32, 32, 3, 3)
    tex[1] = tex[1][:2]
    with pytest.raises(ValueError):
        write("bc7", 32, 32, tex)                                           # layers of unequal level counts
    for layer, level in ((0, 0), (2, 1), (1, 2)):
        tex = _texture("bc7", 32, 32, 3, 3)
        tex[layer][level] = tex[layer][level][:-1]
        with pytest.raises(ValueError):
            write("bc7", 32, 32, tex)                                       # a wrong block count in one (layer, level)
    with pytest.raises(ValueError):
        write("bc7", 32, 32, [])
    write("bc7", 32, 32, _texture("bc7", 32, 32, 7, 1))                    # (7 layers are a fine array)


def test_dds_refuses_formats_without_dxgi_code():
    with pytest.raises(ValueError):
        container.dds_texture_bytes("etc2", 32, 32, _texture("etc2", 32, 32, 2, 1))


# ---- packer: argument errors come back as 1 / 2 with a message, before any device use ----

@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the packer reached the device")
    monkeypatch.setattr(api, "default_context", refuse)
    monkeypatch.setattr(api, "Context", refuse)


def _faces(tmp_path, count, size=(8, 8)):
    paths = []
    for i in range(count):
        p = str(tmp_path / ("face%d.npy" % i))
        np.save(p, np.full(size + (4,), 10 * i, np.uint8))
        paths.append(p)
    return paths


def test_packer_cube_with_five_inputs(tmp_path, no_device, capsys):
    out = str(tmp_path / "out.ktx")
    assert packer.main(["-cube", "-format", "bc7"] + _faces(tmp_path, 5) + [out]) == 1
    assert "6" in capsys.readouterr().err
    assert not (tmp_path / "out.ktx").exists()


def test_packer_inputs_of_different_sizes(tmp_path, no_device, capsys):
    paths = _faces(tmp_path, 2)
    odd = str(tmp_path / "odd.npy")
    np.save(odd, np.zeros((8, 12, 4), np.uint8))
    assert packer.main(["-array", "-format", "bc1"] + paths + [odd, str(tmp_path / "out.ktx")]) == 1
    assert "one size" in capsys.readouterr().err


def test_packer_array_with_r11(tmp_path, no_device, capsys):
    assert packer.main(["-array", "-format", "r11u"] + _faces(tmp_path, 2) + [str(tmp_path / "out.ktx")]) == 1
    assert "r11u" in capsys.readouterr().err


def test_packer_usage_errors(tmp_path, no_device, capsys):
    faces = _faces(tmp_path, 6)
    out = str(tmp_path / "out.ktx")
    assert packer.main(["-array", "-cube"] + faces + [out]) == 2          # one or the other
    assert packer.main(faces + [out]) == 2                                # several inputs need -array or -cube
    assert packer.main(["-array", out]) == 2                              # no input
    assert "-array" in packer.USAGE and "-cube" in packer.USAGE
    assert packer.main(["-cube", "-format", "bc7"] + _faces(tmp_path, 6, (8, 12)) + [out]) == 1   # faces must be square
    stack = str(tmp_path / "stack.npy")
    np.save(stack, np.zeros((5, 8, 8, 4), np.uint8))
    assert packer.main(["-cube", "-format", "bc7", stack, out]) == 1      # a stack of five layers is no cube
    assert packer.main(["-array", "-dds", "-format", "etc2rgb"] + faces + [out]) == 1   # no DXGI code
    capsys.readouterr()
