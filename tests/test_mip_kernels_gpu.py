"""The mip kernels wider than 2x2 on the GPU: cvttmi_build_mips_filtered_device under every kernel, rule, pixel kind and wrap mode
against the numpy restatement (tests/mip_resample_ref.py) in guarded buffers, through pitched and misaligned rows, for texture
arrays, through the encoders and the packer; what the entry points reject; and that a word without kernel bits is what it was."""
import ctypes
import functools

import numpy as np
import pytest

import guarded
import mip_filter_ref
import mip_resample_ref as ref
from convectionkernels_amd import api, container, packer

pytestmark = pytest.mark.gpu

E_INVALID = -1
RGBA8, RGBA16F, SNORM = api.PIXELS_RGBA8, api.PIXELS_RGBA16F, api.PIXELS_RGBA8_SNORM
BOX, SRGB, NORMAL, ALPHA = api.MIP_FILTER_BOX, api.MIP_FILTER_SRGB, api.MIP_FILTER_NORMAL, api.MIP_FILTER_ALPHA_WEIGHTED
POISON = 0xA5

# every (kernel, rule, kind) the entry points take
TRIPLES = [(k, rule, kind) for k in api.MIP_KERNELS for rule, kind in ((BOX, RGBA8), (SRGB, RGBA8), (NORMAL, RGBA8), (BOX, SNORM), (NORMAL, SNORM))]
# 1x1 .. 9x1: every tap lands on one texel / one row; 5x3, 37x10: odd sizes, the last column a neighbour; 64x64, 72x40: 16-byte
# reads in the upper levels; 150x70: level 1 is 75x35, two workgroup tiles (64x16) across and three down, a multiple of neither
SHAPES = [(1, 1), (2, 2), (1, 9), (9, 1), (5, 3), (37, 10), (64, 64), (72, 40), (150, 70)]


def _id(v):
    return {RGBA8: "rgba8", SNORM: "snorm"}[v[2]] + "-" + {BOX: "plain", SRGB: "srgb", NORMAL: "normal"}[v[1]] + "-" + v[0]


@functools.lru_cache(maxsize=None)
def _image(kernel, w, h, kind):
    img, _ = ref.planted_image(kernel, w, h, np.int8 if kind == SNORM else np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _chain(kernel, w, h, kind, word):
    return ref.chain(_image(kernel, w, h, kind), word)


def _expected_pyramid(levels, layout, nbytes):
    exp = np.full(nbytes, POISON, np.uint8)
    for L, level in zip(layout[1:], levels[1:]):
        assert level.shape == (L.height, L.width, 4)
        exp[L.byteOffset: L.byteOffset + level.nbytes] = np.frombuffer(level.tobytes(), np.uint8)
    return exp


def _build(gpu_ctx, view, nbytes, image_ptr, w, h, pitch, kind, levels, word):
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    return api.load_library().cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr() if view is not None else None, nbytes, image_ptr,
                                                                w, h, pitch, kind, levels, word, ctypes.c_void_p(stream))


@pytest.mark.parametrize("triple", TRIPLES, ids=_id)
@pytest.mark.parametrize("w,h", SHAPES)
def test_level_images(gpu_ctx, w, h, triple):
    """every level exact under each wrap mode; the gaps between the levels, the guards and the input untouched"""
    kernel, rule, kind = triple
    layout = api.mip_layout(w, h, 4, 16)
    nbytes = max(layout.pyramid_bytes, 256)
    src, unchanged = guarded.device_input(_image(kernel, w, h, kind))
    for wrap, flag in api.MIP_WRAPS.items():
        word = api.MIP_KERNELS[kernel] | rule | flag
        want = _chain(kernel, w, h, kind, word)
        view, check = guarded.device_buffer(nbytes, poison=POISON, what="pyramid %dx%d %s %s" % (w, h, _id(triple), wrap))
        assert _build(gpu_ctx, view, nbytes, src.data_ptr(), w, h, w * 4, kind, len(layout), word) == 0
        check(_expected_pyramid(want, layout, nbytes))
    unchanged()


def test_planted_footprints_are_in_the_images():
    """(no device work) the images above hold the footprints their helper promises, where the tests rely on them"""
    for w, h in ((64, 64), (72, 40), (150, 70)):
        for kind in (RGBA8, SNORM):
            img, spots = ref.planted_image("lanczos3", w, h, np.int8 if kind == SNORM else np.uint8)
            assert len(spots) == 3 and (img == _image("lanczos3", w, h, kind)).all()
            level = ref.downsample(img, api.MIP_KERNELS["lanczos3"])
            assert [level[y, x, 0] for x, y, _ in spots[:2]] == ([255, 0] if kind == RGBA8 else [127, -128])
            assert (ref.normal_sums(img, api.MIP_KERNELS["lanczos3"] | NORMAL)[spots[2][1], spots[2][0]] == 0).all()


@pytest.mark.parametrize("left", [1, 4])
@pytest.mark.parametrize("triple,wrap", [(("kaiser", SRGB, RGBA8), "repeat"), (("mitchell", NORMAL, SNORM), "mirror"),
                                         (("triangle", BOX, RGBA8), "clamp"), (("lanczos3", NORMAL, RGBA8), "repeat")],
                         ids=lambda v: _id(v) if isinstance(v, tuple) else v)
def test_level_images_through_a_wider_pitch(gpu_ctx, triple, wrap, left):
    """130x66 as a column slice of a 136-texel-wide allocation, starting at its texel 1 (rows off 16-byte boundaries: level 1 is
    read a texel at a time) or 4 (16-byte reads through a pitch); what lies beside the slice must not be read as a neighbour"""
    kernel, rule, kind = triple
    w, h, wide_w = 130, 66, 136
    word = api.MIP_KERNELS[kernel] | rule | api.MIP_WRAPS[wrap]
    want = _chain(kernel, w, h, kind, word)
    wide = np.random.default_rng(5).integers(0, 256, (h, wide_w, 4), dtype=np.uint8).view(want[0].dtype)
    wide[:, left: left + w] = want[0]
    layout = api.mip_layout(w, h, 4, 16)
    src, unchanged = guarded.device_input(wide)
    assert ((src.data_ptr() + left * 4) % 16 != 0) == (left == 1)
    view, check = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr() + left * 4, w, h, wide_w * 4, kind, len(layout), word) == 0
    check(_expected_pyramid(want, layout, layout.pyramid_bytes))
    unchanged()


@pytest.mark.parametrize("triple", TRIPLES, ids=_id)
def test_arrays_equal_build_mips_per_layer(gpu_ctx, triple):
    """three layers two spare rows apart (a layer pitch with a gap): every level of every layer is build_mips of that layer and the
    restatement's bytes"""
    import torch
    kernel, rule, kind = triple
    w, h = 70, 38
    wrap = list(api.MIP_WRAPS)[TRIPLES.index(triple) % 3]
    name = {BOX: "box", SRGB: "srgb", NORMAL: "normal"}[rule]
    layers = [ref.planted_image(kernel, w, h, np.int8 if kind == SNORM else np.uint8, seed=7 + l)[0] for l in range(3)]
    store = torch.full((3, h + 2, w, 4), 0x5A, dtype=torch.uint8, device="cuda").view(torch.int8 if kind == SNORM else torch.uint8)
    store[:, :h] = torch.from_numpy(np.stack(layers)).cuda()
    images = store[:, :h]
    assert images.stride(0) == (h + 2) * w * 4
    got = gpu_ctx.build_mips_array(images, filter=name, kernel=kernel, wrap=wrap)
    assert len(got) == 3
    for l in range(3):
        want = ref.chain(layers[l], api.MIP_KERNELS[kernel] | rule | api.MIP_WRAPS[wrap])
        single = gpu_ctx.build_mips(torch.from_numpy(layers[l].copy()).cuda(), filter=name, kernel=kernel, wrap=wrap)
        assert len(got[l]) == len(want) == len(single)
        for L in range(len(want)):
            assert (got[l][L].cpu().numpy() == want[L]).all(), (l, L)
            assert (single[L].cpu().numpy() == want[L]).all(), (l, L)
    assert (store[:, h:].cpu().numpy().view(np.uint8) == 0x5A).all()


@functools.lru_cache(maxsize=None)
def _photo(w, h):
    rng = np.random.default_rng(w)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (w + h), 255 - x * 255 // w], -1) + rng.integers(-12, 13, (h, w, 4))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("fmt", ["bc1", "bc7"])
def test_encoded_chain_equals_encode_image_of_every_built_level(gpu_ctx, fmt):
    import torch
    w, h = 40, 24
    how = dict(kernel="kaiser", wrap="repeat")
    image = torch.from_numpy(_photo(w, h).copy()).cuda()
    want = ref.chain(_photo(w, h), api.MIP_KERNELS["kaiser"] | SRGB | api.MIP_WRAPS["repeat"])
    levels = gpu_ctx.build_mips(image, filter="srgb", **how)
    assert len(levels) == len(want) == 6
    for l, (got, level) in enumerate(zip(levels, want)):
        assert (got.cpu().numpy() == level).all(), "level %d" % l
    each = [gpu_ctx.encode_image(fmt, level).cpu().numpy() for level in levels]
    packed = gpu_ctx.encode_mips(fmt, image, mip_filter="srgb", **how)
    assert len(packed) == len(each)
    for l, (got, level) in enumerate(zip(packed, each)):
        assert (got.cpu().numpy() == level).all(), "encode_mips level %d" % l
    texture = gpu_ctx.encode_texture(fmt, torch.stack([image, image.flip(0)]), mip_filter="srgb", **how)
    flipped = gpu_ctx.build_mips(image.flip(0).contiguous(), filter="srgb", **how)
    assert len(texture) == 2 and len(texture[0]) == len(each)
    for l in range(len(each)):
        assert (texture[0][l].cpu().numpy() == each[l]).all(), "encode_texture level %d" % l
        assert (texture[1][l].cpu().numpy() == gpu_ctx.encode_image(fmt, flipped[l]).cpu().numpy()).all(), "encode_texture layer 1 level %d" % l
    # the kernel does change the chain
    assert any((a.cpu().numpy() != b.cpu().numpy()).any() for a, b in zip(packed[1:], gpu_ctx.encode_mips(fmt, image, mip_filter="srgb")[1:]))


def test_rejections(gpu_ctx):
    """every rejected word returns the invalid-argument code on the host, before any launch, through all three entry points: the
    pyramid (the output, the work space) keeps its poison and the context has an error text"""
    import torch
    lib = api.load_library()
    w, h = 37, 10
    need = api.mip_layout(w, h, 4, 16).pyramid_bytes
    src, unchanged = guarded.device_input(_image("kaiser", w, h, RGBA8))
    view, check = guarded.device_buffer(need, poison=POISON)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    K, REPEAT, MIRROR = api.MIP_KERNELS, api.MIP_WRAPS["repeat"], api.MIP_WRAPS["mirror"]
    bad = {"wrap without a kernel": [(RGBA8, BOX | REPEAT), (RGBA8, SRGB | MIRROR), (SNORM, NORMAL | REPEAT), (RGBA8, BOX | ALPHA | REPEAT)],
           "both wraps": [(RGBA8, K["kaiser"] | REPEAT | MIRROR), (SNORM, K["triangle"] | NORMAL | REPEAT | MIRROR), (RGBA8, REPEAT | MIRROR)],
           "unknown kernel": [(RGBA8, code << 4) for code in range(5, 16)] + [(RGBA8, 0x50 | SRGB | REPEAT), (SNORM, 0xF0 | NORMAL)],
           "kernel with alpha weights": [(RGBA8, K[k] | f | ALPHA | wr) for k in K for f in (BOX, SRGB) for wr in (0, MIRROR)],
           "kernel with srgb of int8": [(SNORM, K[k] | SRGB) for k in K],
           "kernel with an unknown rule": [(RGBA8, K["mitchell"] | 3), (RGBA8, K["mitchell"] | 0x800), (RGBA8, K["mitchell"] | 0x1000),
                                           (RGBA8, K["mitchell"] | 0x80000000), (SNORM, K["lanczos3"] | NORMAL | ALPHA)]}
    half = dict(w=16, h=4, pitch=128, levels=5)
    for name, words in bad.items():
        for kind, word in words:
            rc = lib.cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr(), need, src.data_ptr(), w, h, w * 4, kind, 6, word, stream)
            assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (name, hex(word))
            rc = lib.cvttmi_build_mips_array_device(gpu_ctx._h, view.data_ptr(), need, src.data_ptr(), w, h, w * 4, w * h * 4, kind, 6, 1, word, stream)
            assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (name, hex(word))
            # one level launches nothing, but the word is still an error
            rc = lib.cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr(), need, src.data_ptr(), w, h, w * 4, kind, 1, word, stream)
            assert rc == E_INVALID, (name, hex(word))
    for k in K:
        for rule in (BOX, SRGB, NORMAL):
            for wr in (0, REPEAT, MIRROR):
                rc = lib.cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr(), need, src.data_ptr(), half["w"], half["h"], half["pitch"],
                                                           RGBA16F, half["levels"], K[k] | rule | wr, stream)
                assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), ("half", k, rule, wr)
    check.untouched()
    unchanged()
    # cvttmi_encode_texture_device: RGBA8 for bc1, RGBA16F for bc6hu
    image = src[: w * h * 4].view(h, w, 4)
    opts = api.Options()
    for fmt, words in (("bc1", [BOX | REPEAT, K["kaiser"] | ALPHA, 0x50, K["kaiser"] | REPEAT | MIRROR]), ("bc6hu", [K["kaiser"], K["triangle"] | REPEAT])):
        fid, bpb = api.TEXTURE_FORMATS[fmt][:2]
        tw, th, texel = (w, h, 4) if fmt == "bc1" else (8, 4, 8)
        sizes = api.texture_layout(tw, th, texel, bpb, 2, 1, api.ORDER_LAYER_MAJOR)
        out, check_out = guarded.device_buffer(sizes.blocks * bpb, poison=POISON)
        work, check_work = guarded.device_buffer(sizes.workBytes, poison=POISON)
        for word in words:
            rc = lib.cvttmi_encode_texture_device(gpu_ctx._h, fid, out.data_ptr(), sizes.blocks * bpb, src.data_ptr(), tw, th, tw * texel,
                                                  tw * th * texel, 1, 2, word, api.ORDER_LAYER_MAJOR, ctypes.addressof(opts), None, None,
                                                  work.data_ptr(), sizes.workBytes, stream)
            assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (fmt, hex(word))
        check_out.untouched()
        check_work.untouched()
    unchanged()
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(image, kernel="cubic")
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(image, wrap="repeat")
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(image, filter="srgb+alpha", kernel="kaiser")
    with pytest.raises(api.CvttError):
        gpu_ctx.build_mips(torch.zeros((4, 4, 4), dtype=torch.float16, device="cuda"), kernel="triangle")
    with pytest.raises(api.CvttError):
        gpu_ctx.encode_mips("bc5s", image, mip_filter="srgb", kernel="kaiser")


@pytest.mark.parametrize("filt", ["box", "srgb+alpha"])
def test_a_word_without_kernel_bits_is_what_it_was(gpu_ctx, filt):
    """the 2x2 rules through the entry point that now knows kernels: the bytes of tests/mip_filter_ref.py, as before"""
    import torch
    w, h = 72, 40
    img = _image("kaiser", w, h, RGBA8)
    want = mip_filter_ref.chain(img, filt)
    layout = api.mip_layout(w, h, 4, 16)
    src, unchanged = guarded.device_input(img)
    view, check = guarded.device_buffer(layout.pyramid_bytes, poison=POISON)
    assert _build(gpu_ctx, view, layout.pyramid_bytes, src.data_ptr(), w, h, w * 4, RGBA8, len(layout), api.MIP_FILTERS[filt]) == 0
    check(_expected_pyramid(want, layout, layout.pyramid_bytes))
    unchanged()
    got = gpu_ctx.build_mips(torch.from_numpy(img.copy()).cuda(), filter=filt, kernel=None, wrap="clamp")
    assert all((a.cpu().numpy() == b).all() for a, b in zip(got, want))


def test_packer_writes_the_chain_under_a_kernel(gpu_ctx, tmp_path, capsys):
    image = _photo(20, 12)
    src, out = str(tmp_path / "src.npy"), str(tmp_path / "out.ktx")
    np.save(src, image)
    assert packer.main(["-format", "bc7", "-mipkernel", "lanczos3", "-mipfilter", "srgb", "-wrap", "mirror", "-metrics", src, out]) == 0
    name, w, h, levels = container.read_ktx_mips(out)
    assert (name, w, h, len(levels)) == ("bc7", 20, 12, 5)  # -mipkernel implies -mips
    want = packer.encode_file_mips(image, "bc7", mip_filter="srgb", kernel="lanczos3", wrap="mirror")
    assert len(want) == 5 and all((a == b).all() for a, b in zip(levels, want))
    plain = packer.encode_file_mips(image, "bc7", mip_filter="srgb")
    assert (levels[0] == plain[0]).all() and any((a != b).any() for a, b in zip(levels[1:], plain[1:]))
    lines = capsys.readouterr().out.strip().split("\n")
    assert [l.split()[:3] for l in lines if l.startswith("mip ")] == [["mip", "1", "10x6"], ["mip", "2", "5x3"], ["mip", "3", "2x1"], ["mip", "4", "1x1"]]
