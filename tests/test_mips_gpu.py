"""Mip chains on the GPU: cvttmi_build_mips_device against the numpy restatement of its three rounding rules (tests/mip_ref.py)
in guarded buffers, Context.encode_mips against encode_image of the reference's level images, what the entry point rejects, and
the packer's -mips files."""
import ctypes
import functools

import numpy as np
import pytest

import guarded
import mip_ref
from convectionkernels_amd import api, container, packer

pytestmark = pytest.mark.gpu

E_INVALID = -1
RGBA8, RGBA16F, SNORM = api.PIXELS_RGBA8, api.PIXELS_RGBA16F, api.PIXELS_RGBA8_SNORM
POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _image(w, h, kind, content="random"):
    """(h, w, 4) test image of a pixel kind, read-only: uint8, int8, or uint16 half bits"""
    rng = np.random.default_rng(1000 * w + 10 * h + kind)
    if kind == RGBA16F:
        img = mip_ref.finite_halfs(rng, (h, w, 4))
        # 2x2 quads of one value each, so that an output texel is exactly that value: -0, +0, the largest halfs, subnormals
        # and the smallest normal (a single row or column reads the same texels through the clamp)
        for i, v in enumerate((0x8000, 0x0000, 0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x0400)):
            if 2 * i < w:
                img[:2, 2 * i: 2 * i + 2] = v
    elif kind == SNORM:
        img = rng.integers(-128, 128, (h, w, 4), dtype=np.int8)
        img[:2, :2] = -128  # a quad of the most negative value
        img[-1, -1] = (-128, 127, -1, 0)
    elif content == "random":
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    else:
        img = np.full((h, w, 4), {"ones": 255, "zeros": 0}[content], np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _chain(w, h, kind, content="random"):
    return mip_ref.chain(_image(w, h, kind, content))


def _texel(kind):
    return 8 if kind == RGBA16F else 4


def _layout(w, h, kind, levels=None):
    return api.mip_layout(w, h, _texel(kind), 16, levels)


def _expected_pyramid(ref, layout, nbytes):
    exp = np.full(nbytes, POISON, np.uint8)
    for L, level in zip(layout[1:], ref[1:]):
        assert level.shape == (L.height, L.width, 4)
        exp[L.byteOffset: L.byteOffset + level.nbytes] = np.frombuffer(level.tobytes(), np.uint8)
    return exp


def _build(gpu_ctx, view, nbytes, image_ptr, w, h, pitch, kind, levels):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    return api.load_library().cvttmi_build_mips_device(gpu_ctx._h, view.data_ptr(), nbytes, image_ptr, w, h, pitch, kind, levels,
                                                       ctypes.c_void_p(stream))


SHAPES = [(1, 1), (2, 2), (1, 9), (9, 1), (5, 3), (37, 10), (64, 64), (72, 40)]


@pytest.mark.parametrize("kind", [RGBA8, SNORM, RGBA16F])
@pytest.mark.parametrize("w,h", SHAPES)
def test_level_images(gpu_ctx, w, h, kind):
    """every level exact, the gaps between the levels, the guards and the input untouched.  1x1 launches nothing; 1x9 / 9x1
    clamp; 5x3 and 37x10 drop an odd row / column; 64x64 and 72x40 start aligned, so their levels of 4 / 2 texels and more per
    row (72x40: level 1, and level 2 of RGBA16F) are made by the 16-byte kernel, the others by the narrow one"""
    ref = _chain(w, h, kind)
    layout = _layout(w, h, kind)
    nbytes = max(layout.pyramid_bytes, 256)
    src, unchanged = guarded.device_input(ref[0])
    view, check = guarded.device_buffer(nbytes, poison=POISON, what="pyramid %dx%d kind %d" % (w, h, kind))
    assert _build(gpu_ctx, view, nbytes, src.data_ptr(), w, h, w * _texel(kind), kind, len(layout)) == 0
    check(_expected_pyramid(ref, layout, nbytes))
    unchanged()


@pytest.mark.parametrize("content", ["ones", "zeros"])
def test_level_images_of_constant_bytes(gpu_ctx, content):
    ref = _chain(37, 10, RGBA8, content)
    assert all((level == ref[0][0, 0, 0]).all() for level in ref)
    layout = _layout(37, 10, RGBA8)
    src, unchanged = guarded.device_input(ref[0])
    view, check = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr(), 37, 10, 37 * 4, RGBA8, len(layout)) == 0
    check(_expected_pyramid(ref, layout, layout.pyramid_bytes))
    unchanged()


@pytest.mark.parametrize("kind", [RGBA8, SNORM, RGBA16F])
def test_level_images_through_a_wider_pitch(gpu_ctx, kind):
    """130x66 as a column slice of a 136-texel-wide allocation, starting at its texel 1: the rows start off 16-byte boundaries,
    so level 1 takes the narrow kernel although its width would allow the wide one; the columns beside the image are not read
    into the result"""
    w, h, left, wide_w = 130, 66, 1, 136
    ref = _chain(w, h, kind)
    rng = np.random.default_rng(5)
    wide = mip_ref.finite_halfs(rng, (h, wide_w, 4)) if kind == RGBA16F else \
        rng.integers(0, 256, (h, wide_w, 4), dtype=np.uint8).view(ref[0].dtype)
    wide[:, left: left + w] = ref[0]
    texel = _texel(kind)
    layout = _layout(w, h, kind)
    src, unchanged = guarded.device_input(wide)
    assert (src.data_ptr() + left * texel) % 16 != 0
    view, check = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr() + left * texel, w, h, wide_w * texel, kind, len(layout)) == 0
    check(_expected_pyramid(ref, layout, layout.pyramid_bytes))
    unchanged()


@pytest.mark.parametrize("w,h", [(258, 2052), (1032, 2052)])
def test_level_images_with_more_rows_than_the_grid(gpu_ctx, w, h):
    """level 1 has 1026 rows and 129 lanes per row: workgroups one row high, more rows than the 1024 workgroups the launch puts
    down the image, so the kernels' row loop runs (258: the narrow kernel; 1032: the wide one)"""
    ref = _chain(w, h, RGBA8)
    layout = _layout(w, h, RGBA8)
    src, unchanged = guarded.device_input(ref[0])
    view, check = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr(), w, h, w * 4, RGBA8, len(layout)) == 0
    check(_expected_pyramid(ref, layout, layout.pyramid_bytes))
    unchanged()


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_fewer_levels_write_only_those(gpu_ctx, levels):
    ref = _chain(37, 10, RGBA8)[:levels]
    full = _layout(37, 10, RGBA8)
    layout = _layout(37, 10, RGBA8, levels)
    src, unchanged = guarded.device_input(ref[0])
    # room for the whole chain: what lies behind the levels asked for stays poison
    view, check = guarded.device_buffer(full.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, full.pyramid_bytes, src.data_ptr(), 37, 10, 37 * 4, RGBA8, levels) == 0
    check(_expected_pyramid(ref, layout, full.pyramid_bytes))
    # ... and exactly the bytes the layout names are enough
    view, check = guarded.device_buffer(max(layout.pyramid_bytes, 4), poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr(), 37, 10, 37 * 4, RGBA8, levels) == 0
    check(_expected_pyramid(ref, layout, max(layout.pyramid_bytes, 4)))
    unchanged()


def test_build_mips_returns_views_of_one_allocation(gpu_ctx):
    import torch
    for kind, dtype in ((RGBA8, torch.uint8), (SNORM, torch.int8), (RGBA16F, torch.int16)):
        ref = _chain(37, 10, kind)
        image = torch.from_numpy(ref[0].view(np.int16).copy() if kind == RGBA16F else ref[0].copy()).cuda()
        levels = gpu_ctx.build_mips(image)
        assert levels[0] is image or levels[0].data_ptr() == image.data_ptr()
        assert len(levels) == 6 and all(l.dtype == dtype for l in levels)
        layout = _layout(37, 10, kind)
        for L, got, want in zip(layout, levels, ref):
            assert tuple(got.shape) == want.shape and (got.cpu().numpy().view(want.dtype) == want).all()
        for L, got in zip(layout[1:], levels[1:]):
            assert got.data_ptr() - levels[1].data_ptr() == L.byteOffset
    # signed=True reads a uint8 image's bytes as int8
    ref = _chain(37, 10, SNORM)
    levels = gpu_ctx.build_mips(torch.from_numpy(ref[0].view(np.uint8).copy()).cuda(), signed=True, levels=3)
    assert len(levels) == 3 and (levels[2].cpu().numpy().view(np.int8) == ref[2]).all()


FORMATS = ["bc1", "bc7", "bc4s", "etc2rgba", "etc2punchthrough", "bc6hu"]


@functools.lru_cache(maxsize=None)
def _format_image(fmt, w, h):
    rng = np.random.default_rng(len(fmt) + w)
    if fmt == "bc6hu":
        return (mip_ref.finite_halfs(rng, (h, w, 4)) & 0x7FFF).astype(np.uint16)
    if fmt == "bc4s":
        return rng.integers(-128, 128, (h, w, 4), dtype=np.int8)
    # smooth colour with noise; punch-through: a transparent region and scattered transparent texels
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (w + h), np.full_like(x, 255)], -1) + rng.integers(-12, 13, (h, w, 4))
    img = np.clip(img, 0, 255).astype(np.uint8)
    if fmt == "etc2punchthrough":
        img[..., 3] = np.where((x < w // 3) | (rng.random((h, w)) < 0.1), 0, 255)
    elif fmt in ("bc7", "etc2rgba"):
        img[..., 3] = rng.integers(0, 256, (h, w))
    return img


@pytest.mark.parametrize("w,h", [(37, 10), (72, 40)])
@pytest.mark.parametrize("fmt", FORMATS)
def test_encoded_chain_equals_encode_image_of_every_level(gpu_ctx, fmt, w, h):
    import torch
    ref = mip_ref.chain(_format_image(fmt, w, h))

    def upload(a):
        return torch.from_numpy(a.view(np.int16).copy() if a.dtype == np.uint16 else a.copy()).cuda()

    got = gpu_ctx.encode_mips(fmt, upload(ref[0]))
    bpb = api.TEXTURE_FORMATS[fmt][1]
    assert len(got) == len(ref)
    for l, (level, packed) in enumerate(zip(ref, got)):
        want = gpu_ctx.encode_image(fmt, upload(level))
        lh, lw = level.shape[:2]
        assert packed.dtype == torch.uint8 and tuple(packed.shape) == (((lw + 3) // 4) * ((lh + 3) // 4), bpb), l
        assert (packed.cpu().numpy() == want.cpu().numpy()).all(), "level %d (%dx%d)" % (l, lw, lh)
    # consecutive in one allocation: a container writer can take it whole
    for a, b in zip(got, got[1:]):
        assert b.data_ptr() == a.data_ptr() + a.numel() and b.untyped_storage().data_ptr() == a.untyped_storage().data_ptr()
    # a shorter chain is the head of the full one
    short = gpu_ctx.encode_mips(fmt, upload(ref[0]), levels=2)
    assert len(short) == 2 and all((a.cpu().numpy() == b.cpu().numpy()).all() for a, b in zip(short, got))


def test_rejections(gpu_ctx):
    """every rejected call returns the invalid-argument code on the host, before any launch: the pyramid keeps its poison and
    the context has an error text"""
    import torch
    lib = api.load_library()
    w, h = 37, 10
    layout = _layout(w, h, RGBA8)
    need = layout.pyramid_bytes
    src, unchanged = guarded.device_input(_image(w, h, RGBA8))
    view, check = guarded.device_buffer(need, poison=POISON)
    img, pyr, pitch = src.data_ptr(), view.data_ptr(), w * 4
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(pyr=pyr, nbytes=need, img=img, w=w, h=h, pitch=pitch, kind=RGBA8, levels=6)
    bad = {
        "null image": dict(img=None), "null pyramid": dict(pyr=None), "no levels": dict(levels=0), "too many levels": dict(levels=7),
        "short pyramid": dict(nbytes=need - 1), "no pyramid bytes": dict(nbytes=0), "pixel kind 3": dict(kind=3),
        "pixel kind -1": dict(kind=-1), "pitch below the row": dict(pitch=w * 4 - 4), "pitch no multiple of the texel": dict(pitch=w * 4 + 2),
        "zero width": dict(w=0), "zero height": dict(h=0), "misaligned image": dict(img=img + 2), "misaligned pyramid": dict(pyr=pyr + 2),
        "misaligned half image": dict(img=img + 4, kind=RGBA16F, w=16, pitch=128, levels=1),
    }
    for name, change in bad.items():
        a = dict(good, **change)
        rc = lib.cvttmi_build_mips_device(gpu_ctx._h, a["pyr"], a["nbytes"], a["img"], a["w"], a["h"], a["pitch"], a["kind"], a["levels"], stream)
        assert rc == E_INVALID, name
        assert lib.cvttmi_last_error(gpu_ctx._h), name
    assert lib.cvttmi_build_mips_device(None, pyr, need, img, w, h, pitch, RGBA8, 6, stream) == E_INVALID
    check.untouched()
    unchanged()
    # the SNORM kind belongs to the mip calls alone
    blocks, check_blocks = guarded.device_buffer(lib.cvttmi_tiled_block_count(w, h) * 64, poison=POISON)
    assert lib.cvttmi_tile_image_device(gpu_ctx._h, blocks.data_ptr(), img, w, h, pitch, SNORM, stream) == E_INVALID
    check_blocks.untouched()
    with pytest.raises(api.CvttError):
        gpu_ctx.encode_mips("r11u", src[: w * h * 4].view(h, w, 4))
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(src[: w * h * 4].view(h, w, 4), levels=7)


def test_python_calls_reject_what_the_single_image_route_rejected(gpu_ctx):
    """encode_mips takes its averaging rule from the format: an int8 image goes with bc4s / bc5s alone.  With bc7 it always was a
    CvttError; with the other formats it used to be averaged as int8, which the one-layer texture call cannot do, so it is
    refused, never averaged as uint8.  Rows that overlap or are no whole texels apart are refused, not copied."""
    import torch
    signed = torch.from_numpy(_image(37, 10, SNORM).copy()).cuda()
    for fmt in ("bc7", "bc1", "bc3", "bc4u", "bc5u", "etc2", "etc2rgba", "bc6hu"):
        with pytest.raises(api.CvttError):
            gpu_ctx.encode_mips(fmt, signed)
    got = gpu_ctx.encode_mips("bc4s", signed)
    want = gpu_ctx.encode_mips("bc4s", signed.view(torch.uint8))  # (the same bytes under the format's rule)
    assert len(got) == 6 and all((a.cpu().numpy() == b.cpu().numpy()).all() for a, b in zip(got, want))
    with pytest.raises(api.CvttError):
        gpu_ctx.encode_mips("nothing", torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda"))  # (format first, as before)
    image = torch.from_numpy(_image(37, 10, RGBA8).copy()).cuda()
    overlapping = torch.as_strided(image, (10, 37, 4), (36 * 4, 4, 1))
    odd = torch.as_strided(torch.zeros(4096, dtype=torch.uint8, device="cuda"), (10, 37, 4), (37 * 4 + 2, 4, 1))
    for bad in (overlapping, odd, image[:1].expand(10, 37, 4)):
        with pytest.raises(api.CvttError):
            gpu_ctx.build_mips(bad)
        with pytest.raises(api.CvttError):
            gpu_ctx.encode_mips("bc1", bad)
    # a wider pitch is taken in place
    window = torch.zeros((10, 40, 4), dtype=torch.uint8, device="cuda")[:, 2:39]
    assert gpu_ctx.build_mips(window)[0].data_ptr() == window.data_ptr()


@pytest.mark.parametrize("fmt,flag,read_mips,read_one", [("bc1", ["-dds"], container.read_dds_mips, container.read_dds),
                                                         ("etc2", [], container.read_ktx_mips, container.read_ktx)])
def test_packer_writes_the_chain(gpu_ctx, tmp_path, capsys, fmt, flag, read_mips, read_one):
    import torch
    image = _format_image("bc1", 37, 10)
    src, out, single = str(tmp_path / "src.npy"), str(tmp_path / "out.bin"), str(tmp_path / "single.bin")
    np.save(src, image)
    assert packer.main(["-format", fmt, "-mips"] + flag + [src, out]) == 0
    assert packer.main(["-format", fmt] + flag + [src, single]) == 0
    name, w, h, levels = read_mips(out)
    assert (name, w, h, len(levels)) == (fmt, 37, 10, 6)
    ctx = api.default_context()
    want = ctx.encode_mips(fmt, torch.from_numpy(image.copy()).cuda())
    for a, b in zip(levels, want):
        assert (a == b.cpu().numpy()).all()
    assert (read_one(out)[3] == read_one(single)[3]).all()
    # -metrics: the lines of level 0 exactly as without -mips, then one line per further level
    capsys.readouterr()
    assert packer.main(["-format", fmt, "-metrics"] + flag + [src, single]) == 0
    plain = capsys.readouterr().out
    assert packer.main(["-format", fmt, "-mips", "-metrics"] + flag + [src, out]) == 0
    lines = capsys.readouterr().out
    assert lines.startswith(plain) and plain
    extra = lines[len(plain):].splitlines()
    assert [l.split()[:3] for l in extra] == [["mip", str(i), "%dx%d" % s] for i, s in enumerate(mip_ref.level_sizes(37, 10)[1:], 1)]
    # ... measured against that level's own image
    images = ctx.build_mips(torch.from_numpy(image.copy()).cuda())
    for l, img, packed in zip(extra, images[1:], want[1:]):
        assert l.split()[3:6] == ["psnr", "%.4f" % ctx.measure_image(fmt, img, packed).psnr(), "dB"], l
