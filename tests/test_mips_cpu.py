"""Mip chains without a GPU: level counts and sizes, cvttmi_mip_layout, the KTX / DDS mip containers and the packer's
argument handling (include/cvtt_mi355x.h "mip chains", container.py, packer.py)."""
import ctypes
import io

import numpy as np
import pytest

import mip_ref
from convectionkernels_amd import api, container, packer

E_INVALID = -1
SIZES = [(1, 1), (2, 2), (5, 3), (1, 9), (37, 10), (256, 256), (16384, 16384)]


def _blocks_of(w, h):
    return ((w + 3) // 4) * ((h + 3) // 4)


def _synthetic_levels(fmt, w, h, levels=None, seed=0):
    rng = np.random.default_rng(seed)
    per = container.FORMATS[fmt][0]
    return [rng.integers(0, 256, (_blocks_of(lw, lh), per), dtype=np.uint8) for lw, lh in mip_ref.level_sizes(w, h)[:levels]]


@pytest.mark.parametrize("w,h", SIZES)
def test_level_counts_and_sizes(w, h):
    sizes = mip_ref.level_sizes(w, h)
    assert api.mip_level_count(w, h) == len(sizes) == int(np.floor(np.log2(max(w, h)))) + 1
    assert sizes[-1] == (1, 1)
    assert [(L.width, L.height) for L in api.mip_layout(w, h, 4, 16)] == sizes
    assert container.mip_sizes(w, h, len(sizes)) == sizes
    if (w, h) == (37, 10):
        assert sizes == [(37, 10), (18, 5), (9, 2), (4, 1), (2, 1), (1, 1)]


def test_level_count_of_an_empty_image_is_zero():
    assert api.mip_level_count(0, 5) == 0 and api.mip_level_count(5, 0) == 0 and api.mip_level_count(0, 0) == 0


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("pixel_bytes,bpb", [(4, 8), (4, 16), (8, 16)])
def test_layout(w, h, pixel_bytes, bpb):
    lib = api.load_library()
    layout = api.mip_layout(w, h, pixel_bytes, bpb)
    end = tiles = blocks = 0
    for l, L in enumerate(layout):
        if l == 0:
            assert (L.byteOffset, L.rowPitchBytes) == (0, 0)  # level 0 stays where the caller has it
        else:
            assert L.byteOffset % 256 == 0 and L.byteOffset >= end and L.byteOffset - end < 256
            assert L.rowPitchBytes == L.width * pixel_bytes
            end = L.byteOffset + L.rowPitchBytes * L.height
        assert L.tileCount == lib.cvttmi_tiled_block_count(L.width, L.height) and L.tileCount % 8 == 0
        assert L.blockCount == _blocks_of(L.width, L.height)
        assert (L.firstTile, L.firstBlock, L.packedByteOffset) == (tiles, blocks, blocks * bpb)
        tiles += L.tileCount
        blocks += L.blockCount
    assert (layout.pyramid_bytes, layout.tile_count, layout.block_count) == (end, tiles, blocks)
    # fewer levels: the same entries, the totals of those levels alone
    for levels in range(1, len(layout)):
        part = api.mip_layout(w, h, pixel_bytes, bpb, levels)
        assert [bytes(a) for a in part] == [bytes(b) for b in layout[:levels]]
        assert part.tile_count == layout[levels].firstTile and part.block_count == layout[levels].firstBlock
        assert part.pyramid_bytes == (0 if levels == 1 else layout[levels - 1].byteOffset + layout[levels - 1].rowPitchBytes * layout[levels - 1].height)


@pytest.mark.parametrize("w,h,kind,bpb,levels", [
    (37, 10, 0, 16, 0), (37, 10, 0, 16, 7), (0, 10, 0, 16, 1), (37, 0, 0, 16, 1), (37, 10, 3, 16, 6), (37, 10, -1, 16, 6),
    (37, 10, 0, 4, 6), (37, 10, 0, 12, 6), (37, 10, 0, 32, 6), (0xFFFFFFFF, 0xFFFFFFFF, 1, 16, 32)])
def test_layout_rejects_bad_arguments_and_writes_nothing(w, h, kind, bpb, levels):
    lib = api.load_library()
    table = (api.MipLevel * 34)()
    ctypes.memset(table, 0xA5, ctypes.sizeof(table))
    assert lib.cvttmi_mip_layout(w, h, kind, bpb, levels, table) == E_INVALID
    assert bytes(table) == b"\xA5" * ctypes.sizeof(table)


def test_layout_takes_the_three_pixel_kinds_and_a_null_table_is_invalid():
    lib = api.load_library()
    table = (api.MipLevel * 7)()
    for kind in (api.PIXELS_RGBA8, api.PIXELS_RGBA16F, api.PIXELS_RGBA8_SNORM):
        assert lib.cvttmi_mip_layout(37, 10, kind, 8, 6, table) == 0
        assert table[1].rowPitchBytes == 18 * (8 if kind == api.PIXELS_RGBA16F else 4)
    assert lib.cvttmi_mip_layout(37, 10, 0, 8, 6, None) == E_INVALID
    with pytest.raises(api.CvttError):
        api.mip_layout(37, 10, 3, 16)  # 3 bytes per texel is no pixel kind


@pytest.mark.parametrize("fmt,kind", [("bc1", "dds"), ("bc7", "dds"), ("etc2", "ktx"), ("etc2rgba", "ktx")])
def test_container_round_trip(fmt, kind, tmp_path):
    to_bytes, write, read, read_one = {
        "dds": (container.dds_mips_bytes, container.write_dds_mips, container.read_dds_mips, container.read_dds),
        "ktx": (container.ktx_mips_bytes, container.write_ktx_mips, container.read_ktx_mips, container.read_ktx)}[kind]
    levels = _synthetic_levels(fmt, 37, 10)
    assert len(levels) == 6
    raw = to_bytes(fmt, 37, 10, levels)
    path = str(tmp_path / ("t." + kind))
    write(path, fmt, 37, 10, levels)
    assert open(path, "rb").read() == raw
    for source in (raw, path):
        name, w, h, got = read(source)
        assert (name, w, h, len(got)) == (fmt, 37, 10, 6)
        for a, b in zip(got, levels):
            assert a.shape == b.shape and (a == b).all()
        # the single-level readers return level 0 of a mip file
        name, w, h, first = read_one(source)
        assert (name, w, h) == (fmt, 37, 10) and (first == levels[0]).all()
    # a shorter chain
    assert len(read(to_bytes(fmt, 37, 10, levels[:3]))[3]) == 3


def test_container_headers():
    import struct
    levels = _synthetic_levels("bc1", 37, 10)
    raw = container.dds_mips_bytes("bc1", 37, 10, levels)
    flags, height, width, linear, _, mips = struct.unpack_from("<6I", raw, 8)
    caps, = struct.unpack_from("<I", raw, 4 + 104)
    assert flags & 0x20000 and mips == 6 and (height, width) == (10, 37) and linear == levels[0].size
    assert caps == 0x1000 | 0x8 | 0x400000
    assert len(raw) == 148 + sum(l.size for l in levels)
    raw = container.ktx_mips_bytes("etc2", 37, 10, levels)
    assert struct.unpack_from("<I", raw, 12 + 4 * 11)[0] == 6
    off = 64
    for l in levels:  # uint32 imageSize, blocks, no padding
        assert struct.unpack_from("<I", raw, off)[0] == l.size
        off += 4 + l.size
    assert off == len(raw)


@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_one_level_chain_is_the_single_level_file(fmt):
    level0 = _synthetic_levels(fmt, 37, 10, 1)
    assert container.dds_mips_bytes(fmt, 37, 10, level0) == container.dds_bytes(fmt, 37, 10, level0[0])
    assert container.ktx_mips_bytes(fmt, 37, 10, level0) == container.ktx_bytes(fmt, 37, 10, level0[0])


@pytest.mark.parametrize("to_bytes", [container.ktx_mips_bytes, container.dds_mips_bytes])
def test_wrong_level_sizes_raise(to_bytes):
    levels = _synthetic_levels("bc1", 37, 10)
    for l in range(6):
        bad = list(levels)
        bad[l] = np.concatenate([bad[l], bad[l][:1]])
        with pytest.raises(ValueError):
            to_bytes("bc1", 37, 10, bad)
    with pytest.raises(ValueError):
        to_bytes("bc1", 37, 10, levels + levels[-1:])  # a seventh level
    with pytest.raises(ValueError):
        to_bytes("bc1", 37, 10, [])
    if to_bytes is container.dds_mips_bytes:
        with pytest.raises(ValueError):
            to_bytes("etc2", 37, 10, levels)  # no DXGI format


def test_pil_reads_level_0_of_the_bc1_mip_dds():
    Image = pytest.importorskip("PIL.Image")
    levels = _synthetic_levels("bc1", 37, 10)
    try:
        one = Image.open(io.BytesIO(container.dds_bytes("bc1", 37, 10, levels[0])))
        one.load()
    except Exception as e:  # this PIL has no DX10 BC1 reader
        pytest.skip("PIL does not open the single-level file: %s" % e)
    chain = Image.open(io.BytesIO(container.dds_mips_bytes("bc1", 37, 10, levels)))
    chain.load()
    assert chain.size == one.size == (37, 10) and (np.array(chain) == np.array(one)).all()


def test_packer_arguments(tmp_path, capsys):
    missing = str(tmp_path / "missing.npy")
    out = str(tmp_path / "out.dds")
    # -mips is a flag: the run gets as far as opening the input (1), not the usage error of an unknown flag (2)
    assert packer.main(["-format", "bc1", "-mips", "-dds", missing, out]) == 1
    assert packer.main(["-format", "bc1", "-mipz", "-dds", missing, out]) == 2
    assert "-mips" in packer.USAGE
    # R11 has no image form: refused before the input is read or anything is encoded
    src = str(tmp_path / "src.npy")
    np.save(src, np.zeros((10, 37, 4), np.uint8))
    capsys.readouterr()
    for fmt in ("r11u", "r11s"):
        assert packer.main(["-mips", "-format", fmt, src, out]) == 1
        assert "-mips" in capsys.readouterr().err
    import os
    assert not os.path.exists(out)
