"""Decoding packed textures and mip chains into linear images on the device (include/cvtt_mi355x.h, "decoding into
images"): cvttmi_decode_image_device / cvttmi_decode_mips_device, Context.decode_image / decode_mips and the unpacker.

Expected images never come from the code under test: the numpy restatement (texture_decode_ref.decode) on seeded random
packed bytes for the 13 formats it covers, the reference decoder's own output (tests/golden/decode.npz) for BC7 and BC6H,
untiled and cropped by untile_ref.untile.  Every output is a guarded buffer (guarded.py): a texel that was not written and a
byte written outside the image -- before it, behind it, between the end of a row and the next pitch, in the alignment gaps of
a pyramid -- are both reported."""
import ctypes
import functools
import os

import numpy as np
import pytest

import guarded
import texture_decode_ref as R
from untile_ref import untile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
IMAGE_FORMATS = [f for f in R.FORMATS if f not in ("r11u", "r11s")]  # every name of the 15 ids with an image form
GEOMETRY_FORMATS = ["bc1", "bc7", "bc6hu"]  # 8-byte blocks to RGBA8, 16-byte blocks to RGBA8, RGBA16F
GOLDEN_KEYS = {"bc7": "bc7", "bc6hu": "bc6u", "bc6hs": "bc6s"}
POISON = 0xA5
E_INVALID = -1
RGBA8, RGBA16F, RGBA8_SNORM = 0, 1, 2


def random_blocks(fmt, n=4096, seed=0):
    """(the generator and seeds of tests/test_decode_formats.py: its CPU tests show that these blocks reach every mode)"""
    bpb = R.FORMATS[fmt][1]
    rng = np.random.Generator(np.random.PCG64(1000 + R.FORMATS[fmt][0] + 97 * seed))
    return rng.integers(0, 256, (n, bpb), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _source(fmt):
    """(packed blocks, their decoded blocks) to cut every test image of `fmt` from; computed once, never modified"""
    if fmt in GOLDEN_KEYS:
        g = np.load(os.path.join(GOLD, "decode.npz"))
        packed, decoded = g[GOLDEN_KEYS[fmt] + "_in"], g[GOLDEN_KEYS[fmt] + "_out"]
    else:
        packed = random_blocks(fmt)
        decoded = R.decode(fmt, packed)
    packed.setflags(write=False)
    decoded.setflags(write=False)
    return packed, decoded


def texel_bytes(fmt):
    return 8 if fmt in ("bc6hu", "bc6hs") else 4


def pixel_kind(fmt):
    return RGBA16F if fmt in ("bc6hu", "bc6hs") else RGBA8


def image_case(fmt, w, h, first=0):
    """(packed blocks, expected (h, w * texel bytes) uint8 rows) of a w x h image made of the source blocks from `first` on"""
    n = ((w + 3) // 4) * ((h + 3) // 4)
    packed, decoded = _source(fmt)
    assert first + n <= len(packed)
    image = untile(decoded[first:first + n], w, h)
    return packed[first:first + n].copy(), image.view(np.uint8).reshape(h, w * texel_bytes(fmt))


def pitched(rows, pitch):
    """the bytes of an image of `rows` (h, row bytes) at `pitch` bytes between rows, the padding holding the poison"""
    h, row = rows.shape
    out = np.full(pitch * (h - 1) + row, POISON, np.uint8)
    for y in range(h):
        out[y * pitch: y * pitch + row] = rows[y]
    return out


def decode_guarded(ctx, fmt, w, h, extra_pitch=0, offset=0, bc_offset=0):
    """cvttmi_decode_image_device into a guarded buffer; checks payload, padding, guards and the input; returns the rows"""
    packed, rows = image_case(fmt, w, h)
    pitch = rows.shape[1] + extra_pitch
    out, check = guarded.device_buffer(pitch * (h - 1) + rows.shape[1], offset, POISON, what="%s %dx%d image" % (fmt, w, h))
    bc, unchanged = guarded.device_input(packed, bc_offset)
    rc = ctx._lib.cvttmi_decode_image_device(ctx._h, R.FORMATS[fmt][0], out.data_ptr(), pitch, pixel_kind(fmt), bc.data_ptr(), w, h, None)
    assert rc == 0, (fmt, w, h, rc, ctx._lib.cvttmi_last_error(ctx._h))
    check(pitched(rows, pitch))
    unchanged()
    got = check.payload()
    return np.stack([got[y * pitch: y * pitch + rows.shape[1]] for y in range(h)])


# 1. every format
@pytest.mark.parametrize("fmt", IMAGE_FORMATS)
def test_every_format(gpu_ctx, fmt):
    assert len(IMAGE_FORMATS) == 16
    decode_guarded(gpu_ctx, fmt, 37, 23)
    # ... and through the Python face: dtype, shape and the same bytes
    import torch
    packed, rows = image_case(fmt, 37, 23)
    image = gpu_ctx.decode_image(fmt, torch.from_numpy(packed).cuda(), 37, 23)
    want = torch.float16 if fmt in ("bc6hu", "bc6hs") else torch.int8 if fmt in ("bc4s", "bc5s") else torch.uint8
    assert image.dtype == want and tuple(image.shape) == (23, 37, 4) and image.is_contiguous()
    assert (image.cpu().numpy().view(np.uint8).reshape(rows.shape) == rows).all()


# 2. geometry: single texels and single blocks, cut blocks, a block row that is no whole group of eight, one block more than
# a wave and one more than a 256-lane workgroup
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (4, 4), (5, 3), (33, 9), (257, 6), (1025, 5)])
@pytest.mark.parametrize("fmt", GEOMETRY_FORMATS)
def test_geometry(gpu_ctx, fmt, size):
    decode_guarded(gpu_ctx, fmt, *size)


# 3. pitch and alignment: the 16-byte path only where base and pitch allow it, the same image either way
@pytest.mark.parametrize("fmt", GEOMETRY_FORMATS)
def test_pitch_and_alignment(gpu_ctx, fmt):
    w, h = 33, 9
    texel = texel_bytes(fmt)
    tight = decode_guarded(gpu_ctx, fmt, w, h)
    assert (decode_guarded(gpu_ctx, fmt, w, h, extra_pitch=texel) == tight).all()  # rows not 16-aligned
    assert (decode_guarded(gpu_ctx, fmt, w, h, extra_pitch=64) == tight).all()
    assert (decode_guarded(gpu_ctx, fmt, w, h, offset=texel) == tight).all()  # base off by one texel
    assert (decode_guarded(gpu_ctx, fmt, w, h, extra_pitch=64, offset=texel) == tight).all()
    # a pitch that keeps every row 16-aligned: the wide path with padding between the rows (33 texels: 132 / 264 bytes a row)
    assert (decode_guarded(gpu_ctx, fmt, w, h, extra_pitch=16 - (w * texel) % 16) == tight).all()
    assert (decode_guarded(gpu_ctx, fmt, w, h, bc_offset=R.FORMATS[fmt][1]) == tight).all()  # d_bc one block into its allocation


# 4. out=
@pytest.mark.parametrize("fmt", GEOMETRY_FORMATS)
def test_out_window(gpu_ctx, fmt):
    import torch
    from convectionkernels_amd import api
    w, h = 33, 9
    texel = texel_bytes(fmt)
    dtype = torch.float16 if texel == 8 else torch.uint8
    packed, rows = image_case(fmt, w, h)
    dev = torch.from_numpy(packed).cuda()
    for first in (0, 4, 5):  # the window's first texel inside the atlas row: 16-aligned or not
        buf, check = guarded.device_buffer(h * 2 * w * texel, 0, POISON, what="%s atlas" % fmt)
        atlas = buf.view(dtype).view(h, 2 * w, 4)
        window = atlas[:, first:first + w]
        assert window.stride(0) == 2 * w * 4 and not window.is_contiguous()
        got = gpu_ctx.decode_image(fmt, dev, w, h, out=window)
        assert got is window
        expected = np.full((h, 2 * w * texel), POISON, np.uint8)
        expected[:, first * texel: (first + w) * texel] = rows
        check(expected)
    good = torch.empty((h, w, 4), dtype=dtype, device="cuda")
    bad = [torch.empty((w, h, 4), dtype=dtype, device="cuda").transpose(0, 1),  # rows and columns swapped
           torch.empty((h, w, 4), dtype=torch.int8 if texel == 4 else torch.int16, device="cuda"),  # the wrong dtype
           torch.empty((h, w + 1, 4), dtype=dtype, device="cuda"), torch.empty((h, w, 4), dtype=dtype),  # wrong shape; a CPU tensor
           torch.empty((h, 4, w), dtype=dtype, device="cuda").transpose(1, 2),  # texels not contiguous
           torch.empty((h, w, 8), dtype=dtype, device="cuda")[:, :, ::2]]
    for out in bad:
        with pytest.raises(api.CvttError):
            gpu_ctx.decode_image(fmt, dev, w, h, out=out)
    # the other argument errors of the Python face: byte count, R11, an unknown name, host blocks
    for args in ((fmt, dev[:-1], w, h), (fmt, dev, w + 4, h), ("r11u", dev, w, h), ("bc9", dev, w, h), (fmt, packed, w, h), (fmt, dev, 0, h)):
        with pytest.raises(api.CvttError):
            gpu_ctx.decode_image(*args, out=good)
    with pytest.raises(api.CvttError):
        gpu_ctx.decode_mips("r11s", [dev], w, h)
    with pytest.raises(api.CvttError):
        gpu_ctx.decode_mips(fmt, [dev, dev], w, h)  # level 1 has another size
    with pytest.raises(api.CvttError):
        gpu_ctx.decode_mips(fmt, [dev] * 7, w, h)  # a 33 x 9 texture has 6 levels


# 5. error codes of the C entries: CVTTMI_E_INVALID, and nothing written
def test_error_codes(gpu_ctx):
    import torch
    from convectionkernels_amd import api
    lib, ctx = gpu_ctx._lib, gpu_ctx._h
    w, h = 33, 9
    out, check = guarded.device_buffer(w * h * 8, 0, POISON, what="image of a refused call")
    layout = api.mip_layout(w, h, 4, 16)
    pyr, check_pyr = guarded.device_buffer(2 * layout.pyramid_bytes, 0, POISON, what="pyramid of a refused call")
    bc = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    o, b, p, pb = out.data_ptr(), bc.data_ptr(), pyr.data_ptr(), layout.pyramid_bytes
    BC7, BC1, BC6HU, BC4S = 0, 1, 2, 9

    def image(fmt=BC1, img=o, pitch=w * 4, pixels=RGBA8, blocks=b, width=w, height=h):
        return lib.cvttmi_decode_image_device(ctx, fmt, img, pitch, pixels, blocks, width, height, None)

    def mips(fmt=BC7, img=o, pitch=w * 4, pyramid=p, pyramid_bytes=pb, pixels=RGBA8, blocks=b, width=w, height=h, levels=len(layout)):
        return lib.cvttmi_decode_mips_device(ctx, fmt, img, pitch, pyramid, pyramid_bytes, pixels, blocks, width, height, levels, None)

    for call in (image, mips):
        assert call(img=None) == E_INVALID
        assert call(blocks=None) == E_INVALID
        assert call(width=0) == E_INVALID
        assert call(height=0) == E_INVALID
        for fmt in (15, 16, 17, -1):
            assert call(fmt=fmt) == E_INVALID, fmt
        assert call(fmt=BC7, pixels=RGBA16F) == E_INVALID
        assert call(fmt=BC6HU, pitch=w * 8, pixels=RGBA8) == E_INVALID
        assert call(fmt=BC4S, pixels=RGBA8_SNORM) == E_INVALID
        assert call(pixels=3) == E_INVALID
        assert call(pitch=w * 4 - 4) == E_INVALID  # below the row
        assert call(pitch=w * 4 + 2) == E_INVALID  # no multiple of the texel
        assert call(fmt=BC6HU, pixels=RGBA16F, pitch=w * 8 + 4) == E_INVALID
        assert call(img=o + 2) == E_INVALID
        assert call(fmt=BC6HU, pixels=RGBA16F, pitch=w * 8, img=o + 4) == E_INVALID
        assert call(fmt=BC1, blocks=b + 4) == E_INVALID
        assert call(fmt=BC7, blocks=b + 8) == E_INVALID
    assert mips(levels=0) == E_INVALID
    assert mips(levels=len(layout) + 1) == E_INVALID
    assert mips(pyramid_bytes=pb - 1) == E_INVALID
    assert mips(pyramid=None) == E_INVALID
    assert mips(pyramid=p + 2) == E_INVALID
    assert lib.cvttmi_decode_image_device(None, BC1, o, w * 4, RGBA8, b, w, h, None) == E_INVALID
    check.untouched()
    check_pyr.untouched()
    # ... and the same arguments without the fault are accepted
    assert image() == 0 and mips() == 0 and mips(levels=1, pyramid=None, pyramid_bytes=0) == 0
    torch.cuda.synchronize()


# 6. mip chains
def mip_case(fmt, w, h):
    """(layout, [packed blocks per level], [expected rows per level]): consecutive source blocks, level after level"""
    from convectionkernels_amd import api
    layout = api.mip_layout(w, h, texel_bytes(fmt), R.FORMATS[fmt][1])
    cases = [image_case(fmt, L.width, L.height, first=L.firstBlock) for L in layout]
    return layout, [c[0] for c in cases], [c[1] for c in cases]


@pytest.mark.parametrize("size,count", [((37, 23), 6), ((8, 1), 4)])
@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_mips(gpu_ctx, fmt, size, count):
    import torch
    w, h = size
    layout, packed, rows = mip_case(fmt, w, h)
    assert len(layout) == count
    fid, bpb = R.FORMATS[fmt][:2]
    # the Python face, from separately allocated levels (concatenated once) and from views of one allocation (used in place)
    whole = torch.from_numpy(np.concatenate(packed)).cuda()
    views = [whole[L.firstBlock: L.firstBlock + L.blockCount] for L in layout]
    for levels in ([torch.from_numpy(p).cuda() for p in packed], views):
        images = gpu_ctx.decode_mips(fmt, levels, w, h)
        assert len(images) == count
        for L, image, level, want in zip(layout, images, levels, rows):
            assert tuple(image.shape) == (L.height, L.width, 4) and image.dtype == torch.uint8
            alone = gpu_ctx.decode_image(fmt, level, L.width, L.height)
            assert torch.equal(image, alone)
            assert (image.cpu().numpy().reshape(want.shape) == want).all()
    # the C entry into guarded buffers: level 0 at a pitch of its own, the pyramid's alignment gaps untouched
    pitch = rows[0].shape[1] + 12
    out, check = guarded.device_buffer(pitch * (h - 1) + rows[0].shape[1], 0, POISON, what="level 0")
    pyr, check_pyr = guarded.device_buffer(layout.pyramid_bytes, 0, POISON, what="pyramid")
    bc, unchanged = guarded.device_input(np.concatenate(packed), bpb)
    rc = gpu_ctx._lib.cvttmi_decode_mips_device(gpu_ctx._h, fid, out.data_ptr(), pitch, pyr.data_ptr(), layout.pyramid_bytes, RGBA8,
                                                bc.data_ptr(), w, h, count, None)
    assert rc == 0
    expected = np.full(layout.pyramid_bytes, POISON, np.uint8)
    for L, want in zip(layout[1:], rows[1:]):
        assert L.rowPitchBytes == want.shape[1] and L.byteOffset % 256 == 0
        expected[L.byteOffset: L.byteOffset + want.size] = want.reshape(-1)
    assert layout.pyramid_bytes > sum(r.size for r in rows[1:])  # (there are gaps)
    check(pitched(rows[0], pitch))
    check_pyr(expected)
    unchanged()
    # fewer levels than the chain has; one level needs no pyramid
    for levels in (count - 1, 1):
        out, check = guarded.device_buffer(rows[0].size, 8, POISON, what="level 0 of %d" % levels)
        sub = api_layout_bytes(fmt, w, h, levels)
        pyr, check_pyr = guarded.device_buffer(max(sub, 1), 0, POISON, what="pyramid of %d" % levels)
        rc = gpu_ctx._lib.cvttmi_decode_mips_device(gpu_ctx._h, fid, out.data_ptr(), rows[0].shape[1], pyr.data_ptr() if levels > 1 else None,
                                                    sub, RGBA8, bc.data_ptr(), w, h, levels, None)
        assert rc == 0
        check(rows[0])
        expected = np.full(max(sub, 1), POISON, np.uint8)
        for L, want in zip(layout[1:levels], rows[1:levels]):
            expected[L.byteOffset: L.byteOffset + want.size] = want.reshape(-1)
        check_pyr(expected)
    assert len(gpu_ctx.decode_mips(fmt, views[:1], w, h)) == 1


def api_layout_bytes(fmt, w, h, levels):
    from convectionkernels_amd import api
    return api.mip_layout(w, h, texel_bytes(fmt), R.FORMATS[fmt][1], levels).pyramid_bytes


def test_mips_hdr(gpu_ctx):
    """an RGBA16F chain: 8-byte texels, the small levels with 8-byte pitches"""
    import torch
    w, h = 37, 23
    layout, packed, rows = mip_case("bc6hu", w, h)
    images = gpu_ctx.decode_mips("bc6hu", [torch.from_numpy(p).cuda() for p in packed], w, h)
    for image, want in zip(images, rows):
        assert image.dtype == torch.float16
        assert (image.cpu().numpy().view(np.uint8).reshape(want.shape) == want).all()


# 7. round trip: the decoded image of an encoded image has exactly the error the measure reports
@pytest.mark.parametrize("fmt", ["bc3", "bc5s"])
def test_round_trip_error_equals_measure(gpu_ctx, fmt):
    import torch
    w, h = 52, 40
    rng = np.random.Generator(np.random.PCG64(52 * 40 + R.FORMATS[fmt][0]))
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 4, y * 6, (x + y) * 2, 255 - x * 3], -1).astype(np.uint8) ^ rng.integers(0, 16, (h, w, 4), dtype=np.uint8)
    dev = torch.from_numpy(img).cuda()
    packed = gpu_ctx.encode_image(fmt, dev)
    decoded = gpu_ctx.decode_image(fmt, packed, w, h).cpu().numpy()
    assert decoded.dtype == (np.int8 if fmt == "bc5s" else np.uint8)
    blocks, valid = R.image_to_blocks(img.view(np.int8) if fmt == "bc5s" else img, fmt)
    source = R.source_values(fmt, blocks)
    values = R.image_to_blocks(decoded, fmt)[0].astype(np.int32)
    diff = (values - source).astype(np.int64)
    mask = R.FORMATS[fmt][2]
    sse = [int((diff[:, :, c] ** 2)[valid].sum()) if mask >> c & 1 else 0 for c in range(4)]
    report = gpu_ctx.measure_image(fmt, dev, packed)
    assert report.texels == w * h
    assert list(report.totals.sse) == sse
    assert sum(sse) > 0


# 8. the unpacker, end to end on the containers the packer writes
@pytest.mark.parametrize("fmt,dds", [("bc7", True), ("etc2rgb", False)])
def test_unpacker_end_to_end(gpu_ctx, tmp_path, fmt, dds):
    import torch
    from convectionkernels_amd import container, packer, unpacker
    w, h = 40, 52
    rng = np.random.Generator(np.random.PCG64(4052))
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 6, y * 4, (x + y) * 2, np.full_like(x, 255)], -1).astype(np.uint8) ^ rng.integers(0, 8, (h, w, 4), dtype=np.uint8)
    np.save(tmp_path / "in.npy", img)
    packed_file = str(tmp_path / ("tex.dds" if dds else "tex.ktx"))
    assert packer.main(["-format", fmt, "-mips"] + (["-dds"] if dds else []) + [str(tmp_path / "in.npy"), packed_file]) == 0
    name, fw, fh, levels = (container.read_dds_mips if dds else container.read_ktx_mips)(packed_file)
    assert (fw, fh, len(levels)) == (w, h, 6) and name == container.canonical(fmt)
    assert unpacker.main(["-mips", packed_file, str(tmp_path / "dec.npy")]) == 0
    sizes = container.mip_sizes(w, h, len(levels))
    for l, ((lw, lh), blocks) in enumerate(zip(sizes, levels)):
        got = np.load(tmp_path / ("dec.%d.npy" % l))
        want = gpu_ctx.decode_image(name, torch.from_numpy(blocks).cuda(), lw, lh).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == (lh, lw, 4) and (got == want).all(), l
    assert not (tmp_path / "dec.6.npy").exists() and not (tmp_path / "dec.npy").exists()
    # one level, by default the first; a level the file does not have
    assert unpacker.main([packed_file, str(tmp_path / "top.npy")]) == 0
    assert (np.load(tmp_path / "top.npy") == np.load(tmp_path / "dec.0.npy")).all()
    assert unpacker.main(["-level", "2", packed_file, str(tmp_path / "two.npy")]) == 0
    assert (np.load(tmp_path / "two.npy") == np.load(tmp_path / "dec.2.npy")).all()
    assert unpacker.main(["-level", "6", packed_file, str(tmp_path / "six.npy")]) == 1
    # an image file for an 8-bit unsigned format
    assert unpacker.main([packed_file, str(tmp_path / "top.png")]) == 0
    from PIL import Image
    assert (np.array(Image.open(tmp_path / "top.png")) == np.load(tmp_path / "top.npy")).all()
