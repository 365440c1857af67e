"""The mip filters on the GPU: cvttmi_build_mips_filtered_device against the numpy restatement (tests/mip_filter_ref.py) in
guarded buffers, every pair of values through the sRGB tables, Context.encode_mips under a filter, the packer's options, and what
the entry point rejects."""
import ctypes
import functools

import numpy as np
import pytest

import guarded
import mip_filter_ref as ref
import mip_ref
from convectionkernels_amd import api, container, packer

pytestmark = pytest.mark.gpu

E_INVALID = -1
RGBA8, RGBA16F, SNORM = api.PIXELS_RGBA8, api.PIXELS_RGBA16F, api.PIXELS_RGBA8_SNORM
BOX, SRGB, NORMAL, ALPHA = api.MIP_FILTER_BOX, api.MIP_FILTER_SRGB, api.MIP_FILTER_NORMAL, api.MIP_FILTER_ALPHA_WEIGHTED
POISON = 0xA5

# every (filter, kind) pair the entry point takes
PAIRS = [(BOX, RGBA8), (BOX, SNORM), (BOX, RGBA16F), (SRGB, RGBA8), (NORMAL, RGBA8), (NORMAL, SNORM), (BOX | ALPHA, RGBA8),
         (SRGB | ALPHA, RGBA8)]
SHAPES = [(1, 1), (2, 2), (1, 9), (9, 1), (5, 3), (37, 10), (64, 64), (72, 40)]


def _planted(kind, rng):
    """quads (a, b, c, d) that meet the rules' special cases"""
    if kind == SNORM:
        z = (0, 0, 0, 0)
        quads = [(z, z, z, z), ((-128,) * 4,) * 4, ((-128, 127, -128, 3), (127, -128, -127, 3), (-128, -128, 1, 3), (127, 127, -1, 3)),
                 ((5, -5, 0, 1), (-5, 5, 0, 1), (7, 0, -7, 1), (-7, 0, 7, 1))]  # Q == 0 away from zero
        for axis in range(3):
            for v in (127, -127, -128):
                t = [0, 0, 0, 9]
                t[axis] = v
                quads.append((tuple(t),) * 4)
        return quads
    c = [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(12)]
    quads = [tuple(c[i] + (0,) for i in range(4)),                                    # nothing to weight by
             tuple(c[i] + (255,) for i in range(4, 8)),                               # all opaque
             (c[8] + (0,), c[9] + (0,), c[10] + (255,), c[11] + (0,)),                # one opaque texel among transparent ones
             ((255, 0, 0, 0), (255, 0, 0, 0), (0, 255, 0, 255), (255, 0, 0, 0)),
             ((255, 255, 255, 1), (0, 0, 0, 0), (0, 0, 0, 0), (255, 255, 255, 0)),    # the smallest weight there is
             ((0, 0, 0, 77), (255, 255, 255, 77), (255, 255, 255, 77), (0, 0, 0, 77)),  # NORMAL: Q == 0
             ((0, 255, 0, 1), (255, 0, 255, 2), (255, 0, 0, 3), (0, 255, 255, 4))]    # ... per channel two of 0 and two of 255
    for axis in range(3):
        for v in (255, 0):
            t = [128, 128, 128, 200]
            t[axis] = v
            quads.append((tuple(t),) * 4)
    return quads


@functools.lru_cache(maxsize=None)
def _image(w, h, kind):
    """(h, w, 4) random image of a pixel kind with the planted quads in as many 2x2 cells as the shape has, read-only"""
    rng = np.random.default_rng(1000 * w + 10 * h + kind)
    if kind == RGBA16F:
        img = mip_ref.finite_halfs(rng, (h, w, 4))
    else:
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8).view(np.int8 if kind == SNORM else np.uint8)
        cells = [(x, y) for y in range(0, h - 1, 2) for x in range(0, w - 1, 2)]
        for (x, y), (a, b, c, d) in zip(cells, _planted(kind, rng)):
            img[y, x], img[y, x + 1], img[y + 1, x], img[y + 1, x + 1] = a, b, c, d
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _chain(w, h, kind, filt):
    return ref.chain(_image(w, h, kind), filt)


def _texel(kind):
    return 8 if kind == RGBA16F else 4


def _expected_pyramid(levels, layout, nbytes):
    exp = np.full(nbytes, POISON, np.uint8)
    for L, level in zip(layout[1:], levels[1:]):
        assert level.shape == (L.height, L.width, 4)
        exp[L.byteOffset: L.byteOffset + level.nbytes] = np.frombuffer(level.tobytes(), np.uint8)
    return exp


def _build(gpu_ctx, view, nbytes, image_ptr, w, h, pitch, kind, levels, filt):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    return api.load_library().cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr() if view is not None else None, nbytes, image_ptr,
                                                                w, h, pitch, kind, levels, filt, ctypes.c_void_p(stream))


@pytest.mark.parametrize("filt,kind", PAIRS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_level_images(gpu_ctx, w, h, filt, kind):
    """every level exact; the gaps between the levels, the guards and the input untouched.  1x9 / 9x1 clamp, 5x3 and 37x10 drop
    an odd row / column, 64x64 and 72x40 take the wide kernel for their upper levels and the narrow one below"""
    want = _chain(w, h, kind, filt)
    layout = api.mip_layout(w, h, _texel(kind), 16)
    nbytes = max(layout.pyramid_bytes, 256)
    src, unchanged = guarded.device_input(want[0])
    view, check = guarded.device_buffer(nbytes, poison=POISON, what="pyramid %dx%d kind %d filter 0x%x" % (w, h, kind, filt))
    assert _build(gpu_ctx, view, nbytes, src.data_ptr(), w, h, w * _texel(kind), kind, len(layout), filt) == 0
    check(_expected_pyramid(want, layout, nbytes))
    unchanged()


def test_planted_quads_meet_the_special_cases():
    """(no device work) the images above do hold what their names say"""
    a, b, c, d = ref.quads(_image(72, 40, RGBA8))
    alpha = a[..., 3] + b[..., 3] + c[..., 3] + d[..., 3]
    assert (alpha == 0).any() and (alpha == 1020).any() and (alpha == 255).any() and (alpha == 1).any()
    s = sum(2 * v[..., :3] - 255 for v in (a, b, c, d))
    assert ((s * s).sum(-1) == 0).sum() >= 2
    a, b, c, d = ref.quads(_image(72, 40, SNORM))
    s = sum(np.maximum(v[..., :3], -127) for v in (a, b, c, d))
    assert ((s * s).sum(-1) == 0).sum() >= 2 and (_image(72, 40, SNORM) == -128).any()


@functools.lru_cache(maxsize=None)
def _pairs_image(with_alpha):
    """512x512: quad (x, y) holds x, x, y, y in the colour channels; alpha 255, or seeded random bytes with 0 and 255 among them"""
    x, y = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    img = np.empty((512, 512, 4), np.uint8)
    for ch in range(3):
        img[0::2, 0::2, ch], img[0::2, 1::2, ch], img[1::2, 0::2, ch], img[1::2, 1::2, ch] = x, x, y, y
    img[..., 3] = 255
    if with_alpha:
        rng = np.random.default_rng(99)
        img[..., 3] = rng.choice(np.array([0, 0, 255, 255, 1, 254] + list(range(256)), np.uint8), (512, 512))
        img[:64:2, :, 3] = 0  # rows of quads whose top texels are transparent ...
        img[64:96, :, 3] = 0  # ... and rows of all-transparent quads
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("filt", ["srgb", "srgb+alpha", "box+alpha"])
def test_every_pair_of_values(gpu_ctx, filt):
    img = _pairs_image(filt != "srgb")
    want = ref.downsample(img, filt)
    if filt == "srgb":
        assert (np.diagonal(want[..., 0]) == np.arange(256)).all()
    layout = api.mip_layout(512, 512, 4, 16, 2)
    src, unchanged = guarded.device_input(img)
    view, check = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr(), 512, 512, 2048, RGBA8, 2, api.MIP_FILTERS[filt]) == 0
    check(_expected_pyramid([img, want], layout, layout.pyramid_bytes))
    unchanged()


@pytest.mark.parametrize("filt,kind", [(SRGB, RGBA8), (NORMAL, RGBA8), (NORMAL, SNORM)])
def test_level_images_through_a_wider_pitch(gpu_ctx, filt, kind):
    """130x66 as a column slice of a 136-texel-wide allocation, starting at its texel 1: the rows start off 16-byte boundaries,
    so level 1 takes the narrow kernel although its width would allow the wide one"""
    w, h, left, wide_w = 130, 66, 1, 136
    want = _chain(w, h, kind, filt)
    wide = np.random.default_rng(5).integers(0, 256, (h, wide_w, 4), dtype=np.uint8).view(want[0].dtype)
    wide[:, left: left + w] = want[0]
    layout = api.mip_layout(w, h, 4, 16)
    src, unchanged = guarded.device_input(wide)
    assert (src.data_ptr() + left * 4) % 16 != 0
    view, check = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr() + left * 4, w, h, wide_w * 4, kind, len(layout), filt) == 0
    check(_expected_pyramid(want, layout, layout.pyramid_bytes))
    unchanged()


@pytest.mark.parametrize("kind", [RGBA8, SNORM, RGBA16F])
def test_box_through_either_entry_is_the_restatement(gpu_ctx, kind):
    """cvttmi_build_mips_device and cvttmi_build_mips_filtered_device under BOX: each held to tests/mip_ref.py on its own"""
    import torch
    w, h = 72, 40
    layout = api.mip_layout(w, h, _texel(kind), 16)
    src, unchanged = guarded.device_input(_image(w, h, kind))
    new, check_new = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    old, check_old = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, new, layout.pyramid_bytes, src.data_ptr(), w, h, w * _texel(kind), kind, len(layout), BOX) == 0
    assert api.load_library().cvttmi_build_mips_device(gpu_ctx._h, old.data_ptr(), layout.pyramid_bytes, src.data_ptr(), w, h, w * _texel(kind),
                                                       kind, len(layout), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    want = _expected_pyramid(mip_ref.chain(_image(w, h, kind)), layout, layout.pyramid_bytes)
    assert (want != POISON).any()
    check_new(want)
    check_old(want)
    unchanged()


@functools.lru_cache(maxsize=None)
def _format_image(fmt, w, h):
    rng = np.random.default_rng(len(fmt) + w)
    y, x = np.mgrid[0:h, 0:w]
    if fmt == "bc5s":  # a bumpy int8 normal map
        n = np.stack([np.sin(x / 3.0), np.cos(y / 2.0), np.full(x.shape, 1.5)], -1)
        n = n / np.sqrt((n * n).sum(-1, keepdims=True))
        img = np.concatenate([np.round(n * 127), np.zeros(x.shape + (1,))], -1) + rng.integers(-3, 4, (h, w, 4))
        return np.clip(img, -128, 127).astype(np.int8)
    img = np.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (w + h), np.zeros_like(x)], -1) + rng.integers(-12, 13, (h, w, 4))
    img = np.clip(img, 0, 255).astype(np.uint8)
    img[..., 3] = np.where(rng.random((h, w)) < 0.3, 0, rng.integers(0, 256, (h, w)))
    return img


@pytest.mark.parametrize("w,h", [(37, 10), (72, 40)])
@pytest.mark.parametrize("fmt,filt", [("bc7", "srgb+alpha"), ("bc1", "srgb+alpha"), ("bc5s", "normal")])
def test_encoded_chain_equals_encode_image_of_every_filtered_level(gpu_ctx, fmt, filt, w, h):
    import torch
    image = torch.from_numpy(_format_image(fmt, w, h).copy()).cuda()
    want = ref.chain(_format_image(fmt, w, h), filt)
    levels = gpu_ctx.build_mips(image, filter=filt)
    assert len(levels) == len(want)
    for l, (got, level) in enumerate(zip(levels, want)):
        assert (got.cpu().numpy() == level).all(), "level %d" % l
    by_value = gpu_ctx.build_mips(image, filter=api.MIP_FILTERS[filt], levels=2)
    assert (by_value[1].cpu().numpy() == want[1]).all()
    packed = gpu_ctx.encode_mips(fmt, image, mip_filter=filt)
    assert len(packed) == len(want)
    for l, (got, level) in enumerate(zip(packed, levels)):
        assert (got.cpu().numpy() == gpu_ctx.encode_image(fmt, level).cpu().numpy()).all(), "level %d" % l
    # the default is the box filter, as before
    assert all((a.cpu().numpy() == b.cpu().numpy()).all() for a, b in zip(gpu_ctx.encode_mips(fmt, image), gpu_ctx.encode_mips(fmt, image, mip_filter="box")))


def test_packer_writes_the_filtered_chain_and_the_mark(gpu_ctx, tmp_path):
    import torch
    image = _format_image("bc7", 37, 10)
    src, out, plain = str(tmp_path / "src.npy"), str(tmp_path / "out.ktx"), str(tmp_path / "plain.ktx")
    np.save(src, image)
    assert packer.main(["-format", "bc7", "-mips", "-mipfilter", "srgb", "-srgb", src, out]) == 0
    assert container.colour_space(out) == "srgb"
    name, w, h, levels = container.read_ktx_mips(out)
    assert (name, w, h, len(levels)) == ("bc7", 37, 10, 6)
    ctx = api.default_context()
    want = ctx.encode_mips("bc7", torch.from_numpy(image.copy()).cuda(), mip_filter="srgb")
    for a, b in zip(levels, want):
        assert (a == b.cpu().numpy()).all()
    # -mipfilter implies -mips; -alphaweight picks the weighted filter; without -srgb the file is unmarked; the mark changes
    # neither level 0 nor the encode
    assert packer.main(["-format", "bc7", "-mipfilter", "srgb", "-alphaweight", src, plain]) == 0
    assert container.colour_space(plain) == "linear"
    got = container.read_ktx_mips(plain)[3]
    want_weighted = ctx.encode_mips("bc7", torch.from_numpy(image.copy()).cuda(), mip_filter="srgb+alpha")
    assert len(got) == 6 and all((a == b.cpu().numpy()).all() for a, b in zip(got, want_weighted))
    assert (got[0] == levels[0]).all()
    assert packer.main(["-format", "bc1", "-dds", "-srgb", src, plain]) == 0
    assert container.colour_space(plain) == "srgb" and len(container.read_dds_mips(plain)[3]) == 1
    assert (container.read_dds(plain)[3] == ctx.encode_image("bc1", torch.from_numpy(image.copy()).cuda()).cpu().numpy()).all()


def test_rejections(gpu_ctx):
    """every rejected call returns the invalid-argument code on the host, before any launch: the pyramid keeps its poison and
    the context has an error text"""
    import torch
    lib = api.load_library()
    w, h = 37, 10
    need = api.mip_layout(w, h, 4, 16).pyramid_bytes
    src, unchanged = guarded.device_input(_image(w, h, RGBA8))
    view, check = guarded.device_buffer(need, poison=POISON)
    img, pyr, pitch = src.data_ptr(), view.data_ptr(), w * 4
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(pyr=pyr, nbytes=need, img=img, w=w, h=h, pitch=pitch, kind=RGBA8, levels=6, filt=SRGB)
    half = dict(kind=RGBA16F, w=16, h=4, pitch=128, levels=5)
    bad = {
        "half srgb": dict(half, filt=SRGB), "half normal": dict(half, filt=NORMAL), "half box+alpha": dict(half, filt=BOX | ALPHA),
        "half srgb+alpha": dict(half, filt=SRGB | ALPHA),
        "snorm srgb": dict(kind=SNORM, filt=SRGB), "snorm box+alpha": dict(kind=SNORM, filt=BOX | ALPHA), "snorm srgb+alpha": dict(kind=SNORM, filt=SRGB | ALPHA),
        "normal+alpha": dict(filt=NORMAL | ALPHA), "snorm normal+alpha": dict(kind=SNORM, filt=NORMAL | ALPHA),
        "filter 3": dict(filt=3), "filter 4": dict(filt=4), "filter 0x200": dict(filt=0x200), "filter 0x1101": dict(filt=0x1101),
        "filter 0xffffffff": dict(filt=0xFFFFFFFF),
        "null image": dict(img=None), "null pyramid": dict(pyr=None), "short pyramid": dict(nbytes=need - 1), "no pyramid bytes": dict(nbytes=0),
        "misaligned image": dict(img=img + 2), "misaligned pyramid": dict(pyr=pyr + 2), "no levels": dict(levels=0),
        "too many levels": dict(levels=7), "pixel kind 3": dict(kind=3), "pitch below the row": dict(pitch=w * 4 - 4), "zero width": dict(w=0),
        # one level launches nothing, but a filter the kind does not take is still an error
        "one level, half srgb": dict(half, filt=SRGB, levels=1),
    }
    for name, change in bad.items():
        a = dict(good, **change)
        rc = lib.cvttmi_build_mips_filtered_device(gpu_ctx._h, a["pyr"], a["nbytes"], a["img"], a["w"], a["h"], a["pitch"], a["kind"],
                                                   a["levels"], a["filt"], stream)
        assert rc == E_INVALID, name
        assert lib.cvttmi_last_error(gpu_ctx._h), name
    assert lib.cvttmi_build_mips_filtered_device(None, pyr, need, img, w, h, pitch, RGBA8, 6, SRGB, stream) == E_INVALID
    check.untouched()
    unchanged()
    image = src[: w * h * 4].view(h, w, 4)
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(image, filter="cubic")
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(image, filter="srgb", signed=True)
    with pytest.raises(api.CvttError):
        gpu_ctx.encode_mips("bc5s", image, mip_filter="srgb+alpha")
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(torch.zeros((4, 4, 4), dtype=torch.float16, device="cuda"), filter="normal")
    check.untouched()
