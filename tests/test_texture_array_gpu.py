"""Texture arrays and cube maps on the GPU: Context.encode_texture against encode_image of every level image the numpy restatement
(tests/mip_filter_ref.py) makes of every layer, the C entry in guarded buffers, cvttmi_build_mips_array_device against the
restatement's level images of every layer, what the entries reject, and packer / unpacker end to end.  (A single image is a texture
of one layer through the same code, so encode_mips / build_mips per layer are no independent reference.)
The shapes are a few hundred blocks: (3, 37x21) has padding tiles to drop, odd sizes and levels narrower than a group down to
1x1; (6, 32x32) is the cube without padding; (2, 260x9) has more than 64 tiles a row, so a wave crosses block rows and levels,
and its height reaches 1 long before its width; (2, 1x1) is one level of one block; (1, 70x5)."""
import ctypes
import functools

import numpy as np
import pytest

import guarded
import mip_filter_ref
from convectionkernels_amd import api, container, packer, unpacker

pytestmark = pytest.mark.gpu

E_INVALID = -1
POISON = 0xA5
RGBA8, RGBA16F, SNORM = api.PIXELS_RGBA8, api.PIXELS_RGBA16F, api.PIXELS_RGBA8_SNORM
BOX, SRGB, NORMAL, ALPHA = api.MIP_FILTER_BOX, api.MIP_FILTER_SRGB, api.MIP_FILTER_NORMAL, api.MIP_FILTER_ALPHA_WEIGHTED
FORMATS = ["bc1", "bc7", "bc6hu", "bc5s", "etc2rgba"]
SHAPES = [(3, 37, 21), (6, 32, 32), (2, 260, 9), (2, 1, 1), (1, 70, 5)]
ORDERS = ["layer", "level"]


@functools.lru_cache(maxsize=None)
def _images(fmt, layers, w, h):
    """(layers, h, w, 4) numpy images of the kind `fmt` is encoded from: smooth ramps with noise, every layer different"""
    rng = np.random.default_rng(7 * layers + 100 * w + h + len(fmt))
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for l in range(layers):
        base = np.stack([(x * (l + 3)) % 256, (y * 11 + 40 * l) % 256, ((x + y) * 5 + 17 * l) % 256, (x * y + 29 * l) % 256], -1)
        img = np.clip(base + rng.integers(-20, 21, (h, w, 4)), 0, 255)
        if fmt in ("bc6hu", "bc6hs"):
            out.append((img / 16.0).astype(np.float16))
        elif fmt in ("bc4s", "bc5s"):
            out.append((img - 128).astype(np.int8))
        else:
            out.append(img.astype(np.uint8))
    res = np.stack(out)
    res.setflags(write=False)
    return res


def _ref_chain(image, filt, levels=None):
    """the restatement's level images of one layer, in the layer's dtype (the restatement reads halfs as uint16 bit patterns)"""
    bits = image.view(np.uint16) if image.dtype == np.float16 else image
    return [level.view(image.dtype) for level in mip_filter_ref.chain(bits, filt, levels)]


@functools.lru_cache(maxsize=None)
def _reference(fmt, layers, w, h, levels=None, mip_filter="box"):
    """[layer][level] numpy blocks: encode_image of every level image the restatement makes of every layer (what
    test_mips_gpu.py holds encode_mips to): computed once, shared, read-only"""
    import torch
    ctx = api.default_context()
    res = []
    for image in _images(fmt, layers, w, h):
        chain = _ref_chain(image, mip_filter, levels)
        res.append([ctx.encode_image(fmt, torch.from_numpy(level.copy()).cuda()).cpu().numpy() for level in chain])
    for chain in res:
        for a in chain:
            a.setflags(write=False)
    return res


def _assert_texture(got, want, what):
    assert len(got) == len(want), what
    for l, (chain, ref) in enumerate(zip(got, want)):
        assert len(chain) == len(ref), (what, l)
        for L, (a, b) in enumerate(zip(chain, ref)):
            a = a.cpu().numpy() if hasattr(a, "cpu") else a
            assert a.shape == b.shape, (what, l, L, a.shape, b.shape)
            bad = (a != b).any(axis=1)
            assert not bad.any(), "%s: layer %d level %d: %d of %d blocks differ, first %d" % (what, l, L, bad.sum(), len(b), np.flatnonzero(bad)[0])


def _ctx():
    return api.default_context()  # the context _reference uses: every comparison is within one context


# ---- 1. bytes ----

@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("layers,w,h", SHAPES)
@pytest.mark.parametrize("fmt", FORMATS)
def test_encode_texture_equals_encode_mips_of_every_layer(gpu_ctx, fmt, layers, w, h, order):
    import torch
    images = torch.from_numpy(_images(fmt, layers, w, h).copy()).cuda()
    got = _ctx().encode_texture(fmt, images, order=order)
    _assert_texture(got, _reference(fmt, layers, w, h), "%s %dx%dx%d %s" % (fmt, layers, w, h, order))
    # the views are the subresources of ONE allocation in the order asked for
    bpb = api.TEXTURE_FORMATS[fmt][1]
    esz = 8 if fmt == "bc6hu" else 4
    assert got.order == order and tuple(got.base.shape) == (api.texture_layout(w, h, esz, bpb, None, layers, order).blocks, bpb)
    for l, chain in enumerate(got):
        for L, t in enumerate(chain):
            first, count = api.texture_subresource(w, h, esz, bpb, None, layers, order, l, L)
            assert t.data_ptr() == got.base.data_ptr() + first * bpb and t.shape[0] == count


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("fmt", FORMATS)
def test_encode_texture_with_fewer_levels(gpu_ctx, fmt, levels, order):
    import torch
    layers, w, h = SHAPES[0]
    images = torch.from_numpy(_images(fmt, layers, w, h).copy()).cuda()
    got = _ctx().encode_texture(fmt, images, levels=levels, order=order)
    _assert_texture(got, _reference(fmt, layers, w, h, levels), "%s %d levels %s" % (fmt, levels, order))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt,mip_filter", [("bc7", "srgb+alpha"), ("bc5s", "normal")])
def test_encode_texture_under_a_filter(gpu_ctx, fmt, mip_filter, order):
    import torch
    layers, w, h = SHAPES[0]
    images = torch.from_numpy(_images(fmt, layers, w, h).copy()).cuda()
    got = _ctx().encode_texture(fmt, images, order=order, mip_filter=mip_filter)
    want = _reference(fmt, layers, w, h, None, mip_filter)
    _assert_texture(got, want, "%s %s %s" % (fmt, mip_filter, order))
    # (the filter matters: some level differs from the box chain's)
    box = _reference(fmt, layers, w, h)
    assert any((a != b).any() for ca, cb in zip(want, box) for a, b in zip(ca, cb))


def test_encode_texture_takes_a_list_and_strided_layers(gpu_ctx):
    import torch
    layers, w, h = SHAPES[0]
    host = _images("bc1", layers, w, h)
    want = _reference("bc1", layers, w, h)
    _assert_texture(_ctx().encode_texture("bc1", [torch.from_numpy(i.copy()).cuda() for i in host]), want, "list")
    # a window of a larger tensor: rows and layers strided, nothing copied
    big = torch.full((layers, h + 3, w + 5, 4), 99, dtype=torch.uint8, device="cuda")
    big[:, 1:h + 1, 2:w + 2] = torch.from_numpy(host.copy()).cuda()
    window = big[:, 1:h + 1, 2:w + 2]
    assert _ctx()._images_in(window)[0].data_ptr() == window.data_ptr()
    _assert_texture(_ctx().encode_texture("bc1", window, order="level"), want, "window")


# ---- 2. buffers, through ctypes on the C entry ----

def _pitched(images, row_extra, layer_extra, poison=0x3C):
    """the images with `row_extra` texels behind every row and `layer_extra` behind every layer, poison in between
    -> (bytes, row pitch, layer pitch)"""
    layers, h, w = images.shape[:3]
    texel = 4 * images.itemsize
    row_pitch = (w + row_extra) * texel
    layer_pitch = h * row_pitch + layer_extra * texel
    raw = np.full(layers * layer_pitch, poison, np.uint8)
    for l in range(layers):
        for y in range(h):
            at = l * layer_pitch + y * row_pitch
            raw[at: at + w * texel] = np.frombuffer(images[l, y].tobytes(), np.uint8)
    return raw, row_pitch, layer_pitch


def _encode_texture_c(ctx, fmt, out, out_bytes, images, w, h, row_pitch, layer_pitch, layers, levels, filt, order, work, work_bytes,
                      options=None, plan=None):
    import torch
    options = options or api.Options()
    plan = plan or api.BC7EncodingPlan()
    return api.load_library().cvttmi_encode_texture_device(
        ctx._h if ctx is not None else None, api.TEXTURE_FORMATS[fmt][0], out, out_bytes, images, w, h, row_pitch, layer_pitch, layers, levels,
        filt, order, ctypes.addressof(options) if options != "null" else None, ctypes.addressof(plan) if plan != "null" else None, None,
        work, work_bytes, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("fmt", ["bc1", "bc7", "bc6hu"])
def test_c_entry_in_guarded_buffers(gpu_ctx, fmt, order):
    layers, w, h = SHAPES[0]
    host = _images(fmt, layers, w, h)
    want = _reference(fmt, layers, w, h)
    levels = len(want[0])
    bpb = api.TEXTURE_FORMATS[fmt][1]
    sizes = api.texture_layout(w, h, 4 * host.itemsize, bpb, levels, layers, order)
    out_bytes = sizes.blocks * bpb
    raw, row_pitch, layer_pitch = _pitched(host, 3, 5)
    src, unchanged = guarded.device_input(raw)
    out, check_out = guarded.device_buffer(out_bytes, poison=POISON, what="d_out")
    work, check_work = guarded.device_buffer(sizes.workBytes, poison=POISON, what="d_work")
    ctx, ov = _ctx(), api.ORDERS[order]
    call = functools.partial(_encode_texture_c, ctx, fmt)
    # a work space one byte short and an output one byte off are refused and leave everything as it was
    assert call(out.data_ptr(), out_bytes, src.data_ptr(), w, h, row_pitch, layer_pitch, layers, levels, BOX, ov, work.data_ptr(), sizes.workBytes - 1) == E_INVALID
    assert call(out.data_ptr(), out_bytes - 1, src.data_ptr(), w, h, row_pitch, layer_pitch, layers, levels, BOX, ov, work.data_ptr(), sizes.workBytes) == E_INVALID
    assert call(out.data_ptr(), out_bytes + 1, src.data_ptr(), w, h, row_pitch, layer_pitch, layers, levels, BOX, ov, work.data_ptr(), sizes.workBytes) == E_INVALID
    assert api.load_library().cvttmi_last_error(ctx._h)
    check_out.untouched()
    check_work.untouched()
    unchanged()
    assert call(out.data_ptr(), out_bytes, src.data_ptr(), w, h, row_pitch, layer_pitch, layers, levels, BOX, ov, work.data_ptr(), sizes.workBytes) == 0
    expected = np.zeros((sizes.blocks, bpb), np.uint8)
    for l in range(layers):
        for L in range(levels):
            first, count = api.texture_subresource(w, h, 4 * host.itemsize, bpb, levels, layers, order, l, L)
            expected[first: first + count] = want[l][L]
    check_out(expected)
    check_work(check_work.payload())  # (the work space's contents are private; its guards are not)
    unchanged()


# ---- 3. layered mips ----

PAIRS = [(BOX, RGBA8), (BOX, SNORM), (BOX, RGBA16F), (SRGB, RGBA8), (NORMAL, RGBA8), (NORMAL, SNORM), (BOX | ALPHA, RGBA8), (SRGB | ALPHA, RGBA8)]


def _kind_images(kind, layers, w, h):
    return _images({RGBA8: "bc7", SNORM: "bc5s", RGBA16F: "bc6hu"}[kind], layers, w, h)


def _build_array_c(ctx, pyramids, nbytes, images, w, h, row_pitch, layer_pitch, kind, levels, layers, filt):
    import torch
    return api.load_library().cvttmi_build_mips_array_device(ctx._h if ctx is not None else None, pyramids, nbytes, images, w, h, row_pitch, layer_pitch,
                                                             kind, levels, layers, filt, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _expected_pyramids(chains, layout, sizes):
    exp = np.full(sizes.pyramidBytes, POISON, np.uint8)
    for l, chain in enumerate(chains):
        for L, level in zip(layout[1:], chain[1:]):
            assert level.shape == (L.height, L.width, 4)
            at = l * sizes.pyramidLayerBytes + L.byteOffset
            exp[at: at + level.nbytes] = np.frombuffer(level.tobytes(), np.uint8)
    return exp


@pytest.mark.parametrize("layers,w,h", [(3, 37, 21), (2, 64, 64)])
@pytest.mark.parametrize("filt,kind", PAIRS)
def test_build_mips_array_equals_build_mips_of_every_layer(gpu_ctx, filt, kind, layers, w, h):
    """(2, 64x64) takes the wide kernel for its upper levels.  Through the Python call, then through the C entry into a guarded
    pyramid of exactly the layout's bytes: the gaps between the levels and the tails between the layers keep their poison."""
    import torch
    host = _kind_images(kind, layers, w, h)
    ctx = _ctx()
    want = [_ref_chain(i, filt) for i in host]
    for i, ref in zip(host, want):  # (build_mips of a layer: the same bytes, as the name says)
        single = ctx.build_mips(torch.from_numpy(i.copy()).cuda(), signed=kind == SNORM, filter=filt)
        assert len(single) == len(ref) and all((a.cpu().numpy().view(np.uint8) == b.view(np.uint8)).all() for a, b in zip(single, ref))
    images = torch.from_numpy(host.copy()).cuda()
    got = ctx.build_mips_array(images, signed=kind == SNORM, filter=filt)
    assert len(got) == layers
    for l, (chain, ref) in enumerate(zip(got, want)):
        assert len(chain) == len(ref)
        assert chain[0].data_ptr() == images[l].data_ptr()  # level 0 is a view of the input
        for L, (a, b) in enumerate(zip(chain, ref)):
            assert (a.cpu().numpy().view(np.uint8) == b.view(np.uint8)).all(), (l, L)
    texel = 4 * host.itemsize
    layout = api.mip_layout(w, h, texel, 16)
    sizes = api.texture_layout(w, h, texel, 16, len(layout), layers)
    raw, row_pitch, layer_pitch = _pitched(host, 4, 8)  # (multiples of 16 bytes: the wide path stays open)
    src, unchanged = guarded.device_input(raw)
    view, check = guarded.device_buffer(sizes.pyramidBytes, poison=POISON, what="pyramids")
    assert _build_array_c(ctx, view.data_ptr(), sizes.pyramidBytes, src.data_ptr(), w, h, row_pitch, layer_pitch, kind, len(layout), layers, filt) == 0
    check(_expected_pyramids(want, layout, sizes))
    unchanged()


@pytest.mark.parametrize("filt", [BOX, SRGB])
def test_layers_off_a_16_byte_boundary(gpu_ctx, filt):
    """(3, 64x8) RGBA8 with a layer pitch of 64 * 4 * 8 + 4 bytes: rows, pitches and widths would allow 16-byte accesses, but layers
    1 and 2 start off a 16-byte boundary, so level 1 must go through the texel-sized kernel for all layers; same bytes"""
    import torch
    layers, w, h = 3, 64, 8
    host = _kind_images(RGBA8, layers, w, h)
    ctx = _ctx()
    want = [[t.cpu().numpy() for t in ctx.build_mips(torch.from_numpy(i.copy()).cuda(), filter=filt)] for i in host]
    layout = api.mip_layout(w, h, 4, 16)
    sizes = api.texture_layout(w, h, 4, 16, len(layout), layers)
    raw, row_pitch, layer_pitch = _pitched(host, 0, 1)
    assert (row_pitch, layer_pitch) == (256, 64 * 4 * 8 + 4)
    src, unchanged = guarded.device_input(raw)
    assert src.data_ptr() % 16 == 0 and (src.data_ptr() + layer_pitch) % 16 == 4
    view, check = guarded.device_buffer(sizes.pyramidBytes, poison=POISON, what="pyramids")
    assert _build_array_c(ctx, view.data_ptr(), sizes.pyramidBytes, src.data_ptr(), w, h, row_pitch, layer_pitch, RGBA8, len(layout), layers, filt) == 0
    check(_expected_pyramids(want, layout, sizes))
    unchanged()
    # the Python call takes the same strided tensor in place
    flat = torch.from_numpy(np.concatenate([raw, np.zeros(4, np.uint8)])).cuda()
    strided = torch.as_strided(flat, (layers, h, w, 4), (layer_pitch, row_pitch, 4, 1))
    assert ctx._images_in(strided)[0].data_ptr() == strided.data_ptr()
    got = ctx.build_mips_array(strided, filter=filt)
    for chain, ref in zip(got, want):
        for a, b in zip(chain, ref):
            assert (a.cpu().numpy() == b).all()
    # ONE layer with that layer pitch: the strides of a single layer say nothing about its rows, so the launch is the one the
    # single-image entry makes of the same image; same bytes, into a pyramid of one layer
    one = api.texture_layout(w, h, 4, 16, len(layout), 1)
    view, check = guarded.device_buffer(one.pyramidBytes, poison=POISON, what="pyramid of one layer")
    assert _build_array_c(ctx, view.data_ptr(), one.pyramidBytes, src.data_ptr(), w, h, row_pitch, layer_pitch, RGBA8, len(layout), 1, filt) == 0
    single, check_single = guarded.device_buffer(one.pyramidBytes, poison=POISON, what="pyramid of the single-image entry")
    assert api.load_library().cvttmi_build_mips_filtered_device(ctx._h, single.data_ptr(), one.pyramidBytes, src.data_ptr(), w, h, row_pitch, RGBA8,
                                                                len(layout), filt, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    check_single(_expected_pyramids(want[:1], layout, one))
    check(check_single.payload())
    unchanged()


# ---- 4. rejections ----

def test_rejections(gpu_ctx):
    """every rejected call returns the invalid-argument code on the host, before any launch: output, work space and pyramids keep
    their poison, the images are unchanged and the context has an error text"""
    import torch
    lib = api.load_library()
    ctx = _ctx()
    layers, w, h = SHAPES[0]
    host = _images("bc7", layers, w, h)
    raw, row_pitch, layer_pitch = _pitched(host, 3, 5)
    src, unchanged = guarded.device_input(raw)
    sizes = api.texture_layout(w, h, 4, 16, 6, layers)
    out, check_out = guarded.device_buffer(sizes.blocks * 16, poison=POISON)
    work, check_work = guarded.device_buffer(sizes.workBytes, poison=POISON)
    good = dict(fmt="bc7", out=out.data_ptr(), out_bytes=sizes.blocks * 16, images=src.data_ptr(), w=w, h=h, row_pitch=row_pitch,
                layer_pitch=layer_pitch, layers=layers, levels=6, filt=BOX, order=0, work=work.data_ptr(), work_bytes=sizes.workBytes)
    bad = {
        "null out": dict(out=None), "null images": dict(images=None), "null work": dict(work=None), "null options": dict(options="null"),
        "null plan for bc7": dict(plan="null"), "no layers": dict(layers=0), "r11u": dict(fmt="r11u"), "r11s": dict(fmt="r11s"),
        "order 2": dict(order=2), "order -1": dict(order=-1), "layer pitch below the image": dict(layer_pitch=h * row_pitch - 4),
        "layer pitch of half a texel": dict(layer_pitch=layer_pitch + 2), "row pitch below the row": dict(row_pitch=4 * w - 4),
        "no levels": dict(levels=0), "too many levels": dict(levels=7), "zero width": dict(w=0), "zero height": dict(h=0),
        "misaligned images": dict(images=src.data_ptr() + 2), "misaligned out": dict(out=out.data_ptr() + 8),
        "misaligned work": dict(work=work.data_ptr() + 16, work_bytes=sizes.workBytes - 16), "short work": dict(work_bytes=sizes.workBytes - 1),
        "out bytes of another order of magnitude": dict(out_bytes=0), "srgb filter for bc5s": dict(fmt="bc5s", filt=SRGB),
        "normal+alpha": dict(filt=NORMAL | ALPHA), "filter 3": dict(filt=3),
    }
    for name, change in bad.items():
        a = dict(good, **change)
        fmt = a.pop("fmt")
        rc = _encode_texture_c(ctx, fmt, a["out"], a["out_bytes"], a["images"], a["w"], a["h"], a["row_pitch"], a["layer_pitch"], a["layers"],
                               a["levels"], a["filt"], a["order"], a["work"], a["work_bytes"], a.get("options"), a.get("plan"))
        assert rc == E_INVALID, name
        assert lib.cvttmi_last_error(ctx._h), name
    # an unknown format id, and no context
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    o, p = api.Options(), api.BC7EncodingPlan()
    for fid in (-1, 17):
        assert lib.cvttmi_encode_texture_device(ctx._h, fid, out.data_ptr(), sizes.blocks * 16, src.data_ptr(), w, h, row_pitch, layer_pitch, layers, 6,
                                                BOX, 0, ctypes.addressof(o), ctypes.addressof(p), None, work.data_ptr(), sizes.workBytes, stream) == E_INVALID
    g = dict(good)
    assert _encode_texture_c(None, "bc7", g["out"], g["out_bytes"], g["images"], w, h, row_pitch, layer_pitch, layers, 6, BOX, 0, g["work"],
                             g["work_bytes"]) == E_INVALID
    check_out.untouched()
    check_work.untouched()

    # cvttmi_build_mips_array_device
    pyr, check_pyr = guarded.device_buffer(sizes.pyramidBytes, poison=POISON)
    good = dict(pyr=pyr.data_ptr(), nbytes=sizes.pyramidBytes, images=src.data_ptr(), w=w, h=h, row_pitch=row_pitch, layer_pitch=layer_pitch,
                kind=RGBA8, levels=6, layers=layers, filt=BOX)
    bad = {
        "null pyramids": dict(pyr=None), "null images": dict(images=None), "no layers": dict(layers=0), "short pyramids": dict(nbytes=sizes.pyramidBytes - 1),
        "one layer's pyramid for three": dict(nbytes=sizes.pyramidLayerBytes), "layer pitch below the image": dict(layer_pitch=h * row_pitch - 4),
        "layer pitch of half a texel": dict(layer_pitch=layer_pitch + 2), "row pitch below the row": dict(row_pitch=4 * w - 4),
        "no levels": dict(levels=0), "too many levels": dict(levels=7), "pixel kind 3": dict(kind=3),
        "half srgb": dict(kind=RGBA16F, filt=SRGB, w=8, h=4, levels=4, layer_pitch=4 * row_pitch + 8),
        "snorm srgb": dict(kind=SNORM, filt=SRGB), "normal+alpha": dict(filt=NORMAL | ALPHA), "misaligned images": dict(images=src.data_ptr() + 2),
        "misaligned pyramids": dict(pyr=pyr.data_ptr() + 2), "one level, snorm srgb": dict(kind=SNORM, filt=SRGB, levels=1),
    }
    for name, change in bad.items():
        a = dict(good, **change)
        rc = _build_array_c(ctx, a["pyr"], a["nbytes"], a["images"], a["w"], a["h"], a["row_pitch"], a["layer_pitch"], a["kind"], a["levels"],
                            a["layers"], a["filt"])
        assert rc == E_INVALID, name
        assert lib.cvttmi_last_error(ctx._h), name
    assert _build_array_c(None, pyr.data_ptr(), sizes.pyramidBytes, src.data_ptr(), w, h, row_pitch, layer_pitch, RGBA8, 6, layers, BOX) == E_INVALID
    check_pyr.untouched()
    unchanged()

    # the Python calls: a tensor that is not on the context's device, a wrong shape, dtype, format, order
    images = torch.from_numpy(host.copy())
    for call in (lambda t: ctx.encode_texture("bc7", t), lambda t: ctx.build_mips_array(t)):
        with pytest.raises(api.CvttError):
            call(images)  # on the CPU
        if torch.cuda.device_count() > 1:
            with pytest.raises(api.CvttError):
                call(images.to("cuda:1"))
        with pytest.raises(api.CvttError):
            call(images.cuda()[0, :, :, :3])
        with pytest.raises(api.CvttError):
            call([images.cuda()[0], images.cuda()[1, :-1]])
    with pytest.raises(api.CvttError):
        ctx.encode_texture("r11u", images.cuda())
    with pytest.raises(api.CvttError):
        ctx.encode_texture("bc6hu", images.cuda())
    with pytest.raises(api.CvttError):
        ctx.encode_texture("bc7", images.cuda(), order="face")
    with pytest.raises(api.CvttError):
        ctx.encode_texture("bc7", images.cuda(), levels=7)


# ---- 5. end to end ----

def test_packer_and_unpacker_end_to_end(gpu_ctx, tmp_path, capsys):
    import torch
    ctx = api.default_context()
    # a cube with its full chain from six .npy faces (20x20: padding tiles in every level), KTX
    faces = _images("bc7", 6, 20, 20)
    paths = []
    for i, face in enumerate(faces):
        paths.append(str(tmp_path / ("face%d.npy" % i)))
        np.save(paths[-1], face)
    cube = str(tmp_path / "cube.ktx")
    capsys.readouterr()
    assert packer.main(["-cube", "-mips", "-metrics", "-format", "bc7"] + paths + [cube]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert [line for line in printed if line.startswith("layer")] == ["layer %d" % n for n in range(6)]
    assert sum(line.startswith("psnr") for line in printed) == 6 and sum(line.startswith("mip ") for line in printed) == 6 * 4
    assert printed[printed.index("layer 1") - 1].startswith("mip 4 1x1 psnr")
    fmt, w, h, layers, is_cube = container.read_ktx_texture(cube)
    assert (fmt, w, h, is_cube, len(layers), len(layers[0])) == ("bc7", 20, 20, True, 6, 5)
    want = ctx.encode_texture("bc7", torch.from_numpy(faces.copy()).cuda(), order="level")
    _assert_texture(layers, [[t.cpu().numpy() for t in chain] for chain in want], "cube.ktx")
    assert struct_u32(cube, 12 + 4 * 9) == 0 and struct_u32(cube, 12 + 4 * 10) == 6  # a single cube: no array elements, six faces
    # a single .npy of shape (L, H, W, 4) gives the same file
    stack, again = str(tmp_path / "faces.npy"), str(tmp_path / "again.ktx")
    np.save(stack, faces)
    assert packer.main(["-cube", "-mips", "-format", "bc7", stack, again]) == 0
    assert open(again, "rb").read() == open(cube, "rb").read()

    # an array of three 37x21 layers, one level, DDS, with metrics per layer
    host = _images("bc1", 3, 37, 21)
    paths = []
    for i, layer in enumerate(host):
        paths.append(str(tmp_path / ("layer%d.npy" % i)))
        np.save(paths[-1], layer)
    array = str(tmp_path / "array.dds")
    capsys.readouterr()
    assert packer.main(["-array", "-dds", "-metrics", "-format", "bc1"] + paths + [array]) == 0
    printed = capsys.readouterr().out.splitlines()
    assert [line for line in printed if line.startswith("layer")] == ["layer 0", "layer 1", "layer 2"]
    assert sum(line.startswith("psnr") for line in printed) == 3
    fmt, w, h, layers, is_cube = container.read_dds_texture(array)
    assert (fmt, w, h, is_cube, len(layers), len(layers[0])) == ("bc1", 37, 21, False, 3, 1)
    want = ctx.encode_texture("bc1", torch.from_numpy(host.copy()).cuda(), levels=1, order="layer")
    _assert_texture(layers, [[t.cpu().numpy() for t in chain] for chain in want], "array.dds")
    # the whole allocation is the file's payload
    assert open(array, "rb").read()[148:] == want.base.cpu().numpy().tobytes()

    # unpacker -layer 1: the image decode_image gives for that layer's blocks
    for path, size, level_args, blocks in ((array, (37, 21), [], layers[1][0]), (cube, (10, 10), ["-level", "1"], container.read_ktx_texture(cube)[3][1][1])):
        out = str(tmp_path / "layer1.npy")
        assert unpacker.main(["-layer", "1"] + level_args + [path, out]) == 0
        image = ctx.decode_image(fmt if path == array else "bc7", torch.from_numpy(blocks.copy()).cuda(), size[0], size[1]).cpu().numpy()
        assert (np.load(out) == image).all()
    assert unpacker.main(["-layer", "3", array, str(tmp_path / "none.npy")]) == 1  # three layers: 0..2
    assert unpacker.main([array, str(tmp_path / "layer0.npy")]) == 0              # the default is layer 0
    assert (np.load(str(tmp_path / "layer0.npy")) == ctx.decode_image("bc1", torch.from_numpy(layers[0][0].copy()).cuda(), 37, 21).cpu().numpy()).all()
    capsys.readouterr()


def struct_u32(path, offset):
    import struct
    with open(path, "rb") as f:
        return struct.unpack_from("<I", f.read(), offset)[0]
