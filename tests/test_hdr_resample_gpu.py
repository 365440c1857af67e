"""RGBA16F under a mip kernel and in a resize on the GPU (include/cvtt_mi355x.h, "RGBA16F under a kernel"): every level and every
resized image bit for bit (uint16) against the numpy float32 restatement (tests/hdr_resample_ref.py), in guarded buffers where the
C entries are called directly; wide and texel reads, subnormals, zeros, planted footprints, a NaN, layers, the encoders, both
resize routes, what the entry points reject, and the packer."""
import ctypes
import functools

import numpy as np
import pytest

import guarded
import hdr_resample_ref as ref
import mip_resample_ref as M
from convectionkernels_amd import api, container, packer, unpacker

pytestmark = pytest.mark.gpu

E_INVALID = -1
RGBA8, HALF, SNORM = api.PIXELS_RGBA8, api.PIXELS_RGBA16F, api.PIXELS_RGBA8_SNORM
K, WRAPS, HDR = api.MIP_KERNELS, api.MIP_WRAPS, api.MIP_HDR
NONNEG, SIGNED = HDR["nonnegative"], HDR["signed"]
POISON = 0xA5
# 134x37: level 1 is 67x18, two tile columns (64) and two tile rows (16), odd sizes; 3x3: the footprint exceeds the image several
# times (mirror among the wraps); 1x9 and 9x1: every tap of one direction lands on one texel
SHAPES = [(134, 37), (3, 3), (1, 9), (9, 1)]


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(bits):
    """uint16 bit patterns -> a float16 CUDA tensor of the same bits"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).cuda().view(torch.float16)


def _bits(tensor):
    import torch
    return tensor.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


@functools.lru_cache(maxsize=None)
def _image(kernel, w, h):
    img, spots = ref.planted_image(kernel, w, h)
    img.setflags(write=False)
    return img, tuple(spots)


@functools.lru_cache(maxsize=None)
def _chain(kernel, w, h, word):
    return ref.chain(_image(kernel, w, h)[0], word)


def _expected_pyramid(levels, layout, nbytes):
    exp = np.full(nbytes, POISON, np.uint8)
    for L, level in zip(layout[1:], levels[1:]):
        assert level.shape == (L.height, L.width, 4) and level.dtype == np.uint16
        exp[L.byteOffset: L.byteOffset + level.nbytes] = np.frombuffer(level.tobytes(), np.uint8)
    return exp


def _build(gpu_ctx, view, nbytes, image_ptr, w, h, pitch, levels, word, kind=HALF):
    return api.load_library().cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr(), nbytes, image_ptr, w, h, pitch, kind, levels, word,
                                                                _stream())


# ---- mip chains ----

@pytest.mark.parametrize("kernel", list(K))
@pytest.mark.parametrize("w,h", SHAPES)
def test_full_chain(gpu_ctx, w, h, kernel):
    """every level exact under both ranges and the three wraps, once from rows and a base on 16-byte boundaries (two texels per
    read) and once through a pitch of 8 w + 8 from a base 8 bytes off them (texel reads); gaps, guards and input untouched"""
    img, spots = _image(kernel, w, h)
    layout = api.mip_layout(w, h, 8, 16)
    nbytes = max(layout.pyramid_bytes, 256)
    tight, tight_unchanged = guarded.device_input(img)
    padded = np.full((h, w + 1, 4), 0x7BFF, np.uint16)  # (a neighbour that would show in every sum it entered)
    padded[:, :w] = img
    loose, loose_unchanged = guarded.device_input(padded, offset=8)
    assert tight.data_ptr() % 16 == 0 and loose.data_ptr() % 16 == 8  # (134 x 8 bytes is a multiple of 16: level 1 of it is read wide)
    for hdr, flag in HDR.items():
        for wrap, wrap_flag in WRAPS.items():
            word = K[kernel] | wrap_flag | flag
            want = _chain(kernel, w, h, word)
            for x, y, sign in (spots if (w, h) == SHAPES[0] else ()):
                assert want[1][y, x].tolist() == [0x7BFF if sign > 0 else (0xFBFF if flag == SIGNED else 0)] * 4
            for src, pitch in ((tight, 8 * w), (loose, 8 * w + 8)):
                view, check = guarded.device_buffer(nbytes, poison=POISON, what="pyramid %dx%d %s %s %s pitch %d" % (w, h, kernel, hdr, wrap, pitch))
                assert _build(gpu_ctx, view, nbytes, src.data_ptr(), w, h, pitch, len(layout), word) == 0
                check(_expected_pyramid(want, layout, nbytes))
    tight_unchanged()
    loose_unchanged()
    assert len(spots) == (2 if (w, h) == SHAPES[0] else 0)


@pytest.mark.parametrize("hdr", list(HDR))
def test_subnormals_zeros_and_random_bits(gpu_ctx, hdr):
    """images of subnormal halfs only (0x0001 .. 0x03FF, and the same with signs), of +-0 only, and of random finite bit patterns:
    half subnormals are read and produced, not flushed, and no -0 comes out of a sum"""
    rng = np.random.default_rng(17)
    w, h = 70, 21
    sub = rng.integers(1, 0x400, (h, w, 4), dtype=np.uint16)
    images = {"subnormal": sub, "signed subnormal": sub | (rng.integers(0, 2, (h, w, 4), dtype=np.uint16) << 15),
              "zeros": rng.integers(0, 2, (h, w, 4), dtype=np.uint16) << 15, "bits": ref.random_finite(rng, (h, w, 4))}
    for name, img in images.items():
        for kernel, wrap in (("lanczos3", "clamp"), ("mitchell", "mirror")):
            got = gpu_ctx.build_mips(_cuda(img), kernel=kernel, wrap=wrap, hdr=hdr)
            want = ref.chain(img, K[kernel] | WRAPS[wrap] | HDR[hdr])
            assert len(got) == len(want)
            for l in range(1, len(want)):
                assert (_bits(got[l]) == want[l]).all(), (name, kernel, l)
            if name == "zeros":
                assert all((level == 0).all() for level in want[1:])
            if name == "subnormal":
                assert ((want[1] & 0x7C00) == 0).mean() > 0.5  # most results are subnormal halfs themselves


def test_one_nan_texel(gpu_ctx):
    """only the texels whose footprint holds the NaN are affected, and they are NaN"""
    rng = np.random.default_rng(23)
    w, h, nx, ny = 40, 24, 21, 9
    img = (rng.uniform(0.0, 4.0, (h, w, 4))).astype(np.float16).view(np.uint16)
    img[ny, nx] = 0x7E00
    word = K["lanczos3"] | SIGNED
    got = _bits(gpu_ctx.build_mips(_cuda(img), levels=2, kernel="lanczos3", hdr="signed")[1])
    want = ref.downsample(img, word)
    hit = (M.footprint(h, 12, 0) == ny).any(axis=1)[:, None] & (M.footprint(w, 12, 0) == nx).any(axis=1)[None, :]
    assert hit.sum() == 36
    is_nan = (got & 0x7FFF) > 0x7C00
    assert (is_nan == hit[..., None]).all() and (is_nan == ((want & 0x7FFF) > 0x7C00)).all()
    assert (got[~hit] == want[~hit]).all()


def test_layers_equal_build_mips_per_layer(gpu_ctx):
    """three layers two spare rows apart (a padded layer pitch): every level of every layer is build_mips of that layer"""
    import torch
    w, h = 70, 38
    layers = [ref.planted_image("kaiser", w, h, seed=7 + l)[0] for l in range(3)]
    store = torch.full((3, h + 2, w, 4), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.float16)
    store[:, :h] = _cuda(np.stack(layers))
    images = store[:, :h]
    assert images.stride(0) == (h + 2) * w * 4
    got = gpu_ctx.build_mips_array(images, kernel="kaiser", wrap="repeat", hdr="signed")
    for l in range(3):
        want = ref.chain(layers[l], K["kaiser"] | WRAPS["repeat"] | SIGNED)
        single = gpu_ctx.build_mips(_cuda(layers[l]), kernel="kaiser", wrap="repeat", hdr="signed")
        assert len(got[l]) == len(want) == len(single)
        for L in range(len(want)):
            assert (_bits(got[l][L]) == want[L]).all() and (_bits(single[L]) == want[L]).all(), (l, L)
    assert (_bits(store[:, h:]) == 0x5A5A).all()


def _radiance(w, h, signed, seed=0):
    """a smooth HDR image with highlights (and, signed, negative texels), float16 bits"""
    rng = np.random.default_rng(w + 100 * h + seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([0.2 + x / w, 0.1 + y / h, 0.5 + (x + y) / (w + h), np.ones_like(x, float)], -1) * np.exp(rng.normal(0.0, 1.0, (h, w, 1)))
    img[rng.integers(0, h, 6), rng.integers(0, w, 6), :3] = 900.0
    if signed:
        img[..., :3] -= 0.6
    return img.astype(np.float16).view(np.uint16)


@pytest.mark.parametrize("fmt,hdr", [("bc6hu", "nonnegative"), ("bc6hs", "signed")])
def test_encoded_chain_equals_encode_image_of_every_built_level(gpu_ctx, fmt, hdr):
    import torch
    bits = _radiance(20, 12, fmt == "bc6hs")
    image = _cuda(bits)
    want = ref.chain(bits, K["lanczos3"] | HDR[hdr])
    levels = gpu_ctx.build_mips(image, kernel="lanczos3", hdr=hdr)
    assert len(levels) == len(want) == 5 and all((_bits(a) == b).all() for a, b in zip(levels, want))
    each = [gpu_ctx.encode_image(fmt, level).cpu().numpy() for level in levels]
    packed = gpu_ctx.encode_mips(fmt, image, kernel="lanczos3", hdr=hdr)
    assert len(packed) == len(each) and all((a.cpu().numpy() == b).all() for a, b in zip(packed, each))
    # the kernel does change the chain, and without a range it stays refused
    assert any((a.cpu().numpy() != b.cpu().numpy()).any() for a, b in zip(packed[1:], gpu_ctx.encode_mips(fmt, image)[1:]))
    with pytest.raises(api.CvttError):
        gpu_ctx.encode_mips(fmt, image, kernel="lanczos3")
    # a cube of 8x8 faces, both orders
    faces = np.stack([_radiance(8, 8, fmt == "bc6hs", seed=f) for f in range(6)])
    cube = _cuda(faces)
    built = gpu_ctx.build_mips_array(cube, kernel="lanczos3", wrap="mirror", hdr=hdr)
    for order in ("layer", "level"):
        texture = gpu_ctx.encode_texture(fmt, cube, order=order, kernel="lanczos3", wrap="mirror", hdr=hdr)
        assert len(texture) == 6 and all(len(t) == 4 for t in texture)
        for f in range(6):
            for l in range(4):
                assert (texture[f][l].cpu().numpy() == gpu_ctx.encode_image(fmt, built[f][l]).cpu().numpy()).all(), (order, f, l)
    torch.cuda.synchronize()


# ---- resize ----

def _work_bytes(w, h, dw, dh, word, layers=1):
    need = ctypes.c_size_t(0)
    assert api.load_library().cvttmi_resize_work_bytes(w, h, dw, dh, HALF, word, layers, ctypes.byref(need)) == 0
    return need.value


def _resize_guarded(gpu_ctx, images, dw, dh, word, src_gap=(0, 0), dst_gap=(0, 0), what=""):
    """the C call on (L, H, W, 4) uint16 images through guarded buffers, rows `gap[0]` texels and layers `gap[1]` rows further apart
    than they need be: the (L, dh, dw, 4) result, after checking that exactly dw x 8 bytes of each row were written and nothing else
    -- the pitch gaps and guards of the destination, the guards of the work space, the source"""
    n, h, w = images.shape[:3]
    src_row, dst_row = 8 * (w + src_gap[0]), 8 * (dw + dst_gap[0])
    src_layer, dst_layer = src_row * (h + src_gap[1]), dst_row * (dh + dst_gap[1])
    held = np.full((n, h + src_gap[1], w + src_gap[0], 4), 0x7BFF, np.uint16)
    held[:, :h, :w] = images
    src, unchanged = guarded.device_input(held)
    dst, check = guarded.device_buffer(n * dst_layer, poison=POISON, what="resized " + what)
    need = _work_bytes(w, h, dw, dh, word, n)
    work, check_work = guarded.device_buffer(need, poison=POISON, what="work space " + what)
    rc = api.load_library().cvttmi_resize_image_device(gpu_ctx._h, dst.data_ptr(), dw, dh, dst_row, dst_layer, src.data_ptr(), w, h, src_row,
                                                       src_layer, HALF, n, word, work.data_ptr(), need, _stream())
    assert rc == 0, gpu_ctx._lib.cvttmi_last_error(gpu_ctx._h)
    got = check.payload().view(np.uint16).reshape(n, dh + dst_gap[1], dw + dst_gap[0], 4)
    expected = np.full_like(got, POISON * 0x0101)
    expected[:, :dh, :dw] = got[:, :dh, :dw]
    check(expected)
    check_work(check_work.payload())
    unchanged()
    return got[:, :dh, :dw].copy()


@functools.lru_cache(maxsize=None)
def _tables(w, h, dw, dh, kernel):
    """what the C function returned: the restatement computes with these"""
    return api.resize_taps(w, dw, kernel), api.resize_taps(h, dh, kernel)


def _want(img, dw, dh, kernel, hdr, wrap="clamp"):
    h, w = img.shape[:2]
    return ref.resize(img, dw, dh, kernel, hdr, wrap, tables=_tables(w, h, dw, dh, kernel))


@functools.lru_cache(maxsize=None)
def _random(w, h, seed=0):
    img = ref.random_finite(np.random.default_rng(7 * w + h + 1000 * seed), (h, w, 4))
    img.setflags(write=False)
    return img


SIZES = [((37, 29), (16, 12)), ((37, 29), (64, 48)), ((37, 29), (37, 29)), ((6, 700), (5, 3))]


@pytest.mark.parametrize("hdr", list(HDR))
@pytest.mark.parametrize("sizes", SIZES, ids=lambda v: "%dx%d-%dx%d" % (v[0] + v[1]))
def test_resize_bits_of_the_restatement(gpu_ctx, sizes, hdr):
    """down, up, the same size, and a footprint of 1400 rows: the first three in one launch through LDS, the last in two"""
    (w, h), (dw, dh) = sizes
    img = _random(w, h)
    assert api.resize_launches(w, h, dw, dh, "lanczos3", hdr=hdr) == (2 if (w, h) == (6, 700) else 1)
    got = _resize_guarded(gpu_ctx, img[None], dw, dh, K["lanczos3"] | HDR[hdr], src_gap=(1, 0), dst_gap=(3, 0), what="%s %s" % (sizes, hdr))
    assert (got[0] == _want(img, dw, dh, "lanczos3", hdr)).all()


@pytest.mark.parametrize("kernel", list(api.RESIZE_KERNELS))
def test_resize_kernels_wraps_and_layers(gpu_ctx, kernel):
    """the five kernels (the area box included) under the three wraps, two layers a padded pitch apart, on both routes"""
    for (w, h), (dw, dh), hdr in (((37, 29), (16, 12), "signed"), ((6, 300), (5, 3), "nonnegative")):
        images = np.stack([_random(w, h, seed=1), _random(w, h, seed=2)])
        for wrap, wrap_flag in WRAPS.items():
            word = api.RESIZE_KERNELS[kernel] | wrap_flag | HDR[hdr]
            got = _resize_guarded(gpu_ctx, images, dw, dh, word, src_gap=(0, 2), dst_gap=(1, 1), what="%s %s" % (kernel, wrap))
            for l in range(2):
                assert (got[l] == _want(images[l], dw, dh, kernel, hdr, wrap)).all(), (kernel, wrap, l, (w, h))
    assert api.resize_launches(6, 300, 5, 3, kernel, hdr="nonnegative") == 2 and api.resize_launches(37, 29, 16, 12, kernel, hdr="signed") == 1


def test_resize_through_the_api(gpu_ctx):
    """Context.resize: a result of its own, out= into a strided float16 view whose neighbours keep their poison, exactly half the
    size = the mip kernel's level, the same size = the image"""
    import torch
    img = _random(37, 29, seed=3)
    got = gpu_ctx.resize(_cuda(img), 16, 12, kernel="kaiser", wrap="mirror", hdr="signed")
    assert got.dtype == torch.float16 and tuple(got.shape) == (12, 16, 4)
    assert (_bits(got) == _want(img, 16, 12, "kaiser", "signed", "mirror")).all()
    atlas = torch.full((2, 20, 40, 4), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.float16)
    window = atlas[:, 3:15, 8:24]
    pair = np.stack([img, _random(37, 29, seed=4)])
    assert gpu_ctx.resize(_cuda(pair), 16, 12, hdr="nonnegative", out=window) is window
    after = _bits(atlas)
    for l in range(2):
        assert (after[l, 3:15, 8:24] == _want(pair[l], 16, 12, "lanczos3", "nonnegative")).all()
    after[:, 3:15, 8:24] = 0x5A5A
    assert (after == 0x5A5A).all()
    # exactly half
    even = _random(64, 40, seed=5)
    for kernel in K:
        for hdr in HDR:
            level = gpu_ctx.build_mips(_cuda(even), levels=2, kernel=kernel, wrap="repeat", hdr=hdr)[1]
            assert (_bits(gpu_ctx.resize(_cuda(even), 32, 20, kernel=kernel, wrap="repeat", hdr=hdr)) == _bits(level)).all(), (kernel, hdr)
    # the same size: the image, under SIGNED without -0 and under NONNEGATIVE without a sign
    no_negative_zero = np.where(img == 0x8000, 0, img)
    assert (_bits(gpu_ctx.resize(_cuda(no_negative_zero), 37, 29, kernel="mitchell", hdr="signed")) == no_negative_zero).all()
    assert (_bits(gpu_ctx.resize(_cuda(img & 0x7FFF), 37, 29, kernel="box", hdr="nonnegative")) == img & 0x7FFF).all()
    for call in (lambda: gpu_ctx.resize(_cuda(img), 16, 12), lambda: gpu_ctx.resize(_cuda(img), 16, 12, filter="srgb", hdr="signed"),
                 lambda: gpu_ctx.resize(torch.zeros((4, 4, 4), dtype=torch.uint8, device="cuda"), 2, 2, hdr="signed"),
                 lambda: gpu_ctx.resize(_cuda(img), 16, 12, hdr="signed", out=torch.zeros((12, 16, 4), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(api.CvttError):
            call()


# ---- what the entry points reject ----

def test_rejections(gpu_ctx):
    """E_INVALID with an error text on the host, before any launch, through all four entry points: outputs and work space keep
    their poison"""
    import torch
    lib = api.load_library()
    w, h = 16, 8
    stream = _stream()
    need = api.mip_layout(w, h, 8, 16).pyramid_bytes
    src, unchanged = guarded.device_input(_random(w, h))
    view, check = guarded.device_buffer(need, poison=POISON)
    ok = K["lanczos3"] | NONNEG
    half_words = {"both flags": [K["lanczos3"] | NONNEG | SIGNED, K["kaiser"] | 0x200 | NONNEG | SIGNED],
                  "no flag": [K["lanczos3"], K["triangle"] | 0x400],
                  "a flag with SRGB / NORMAL / ALPHA_WEIGHTED": [ok | 1, K["kaiser"] | SIGNED | 2, ok | 0x100],
                  "0x800 and other bits": [ok | 0x800, K["lanczos3"] | 0x800, ok | 0x4000, ok | 0x80000000],
                  "both wraps, an unknown kernel": [ok | 0x600, 0x50 | NONNEG]}
    mip_only = {"a flag without a kernel": [NONNEG, SIGNED, NONNEG | SIGNED, NONNEG | 0x200]}
    byte_words = {"a flag with RGBA8 / SNORM": [(RGBA8, ok), (RGBA8, K["kaiser"] | SIGNED), (SNORM, ok), (RGBA8, NONNEG), (SNORM, K["mitchell"] | SIGNED | 2),
                                                (RGBA8, ok | 1)]}
    cases = [(HALF, word, name) for name, words in list(half_words.items()) + list(mip_only.items()) for word in words] + \
            [(kind, word, name) for name, words in byte_words.items() for kind, word in words]
    for kind, word, name in cases:
        texel = 8 if kind == HALF else 4
        rc = lib.cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr(), need, src.data_ptr(), w, h, w * texel, kind, 4, word, stream)
        assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (name, hex(word))
        rc = lib.cvttmi_build_mips_array_device(gpu_ctx._h, view.data_ptr(), need, src.data_ptr(), w, h, w * texel, w * h * texel, kind, 4, 1, word,
                                                stream)
        assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (name, hex(word))
        rc = lib.cvttmi_build_mips_filtered_device(gpu_ctx._h, view.data_ptr(), need, src.data_ptr(), w, h, w * texel, kind, 1, word, stream)
        assert rc == E_INVALID, (name, hex(word))
    # misaligned 8-byte pointers and pitches
    for args in ((view.data_ptr(), src.data_ptr() + 4, w * 8), (view.data_ptr() + 4, src.data_ptr(), w * 8), (view.data_ptr(), src.data_ptr(), w * 8 + 4)):
        rc = lib.cvttmi_build_mips_filtered_device(gpu_ctx._h, args[0], need - 8, args[1], w - 1, h, args[2], HALF, 4, ok, stream)
        assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), args
    check.untouched()
    # cvttmi_encode_texture_device
    opts = api.Options()
    fid, bpb = api.TEXTURE_FORMATS["bc6hu"][:2]
    sizes = api.texture_layout(w, h, 8, bpb, 3, 1, api.ORDER_LAYER_MAJOR)
    out, check_out = guarded.device_buffer(sizes.blocks * bpb, poison=POISON)
    work, check_work = guarded.device_buffer(sizes.workBytes, poison=POISON)
    for kind, word, name in cases:
        if kind != HALF:
            continue
        rc = lib.cvttmi_encode_texture_device(gpu_ctx._h, fid, out.data_ptr(), sizes.blocks * bpb, src.data_ptr(), w, h, w * 8, w * h * 8, 1, 3, word,
                                              api.ORDER_LAYER_MAJOR, ctypes.addressof(opts), None, None, work.data_ptr(), sizes.workBytes, stream)
        assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (name, hex(word))
    # ... and a flag with a format of RGBA8 images
    fid1, bpb1 = api.TEXTURE_FORMATS["bc1"][:2]
    sizes1 = api.texture_layout(w, h, 4, bpb1, 3, 1, api.ORDER_LAYER_MAJOR)
    assert sizes1.blocks * bpb1 <= sizes.blocks * bpb and sizes1.workBytes <= sizes.workBytes
    rc = lib.cvttmi_encode_texture_device(gpu_ctx._h, fid1, out.data_ptr(), sizes1.blocks * bpb1, src.data_ptr(), w, h, w * 4, w * h * 4, 1, 3, ok,
                                          api.ORDER_LAYER_MAJOR, ctypes.addressof(opts), None, None, work.data_ptr(), sizes1.workBytes, stream)
    assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h)
    check_out.untouched()
    check_work.untouched()
    # cvttmi_resize_image_device
    dw, dh = 8, 4
    dst, check_dst = guarded.device_buffer(dw * dh * 8, poison=POISON)
    work_bytes = _work_bytes(w, h, dw, dh, ok)
    rwork, check_rwork = guarded.device_buffer(work_bytes + 4096, poison=POISON)
    for kind, word, name in cases:
        if name in mip_only:
            continue
        texel = 8 if kind == HALF else 4
        rc = lib.cvttmi_resize_image_device(gpu_ctx._h, dst.data_ptr(), dw, dh, dw * texel, dw * dh * texel, src.data_ptr(), w, h, w * texel,
                                            w * h * texel, kind, 1, word, rwork.data_ptr(), work_bytes + 4096, stream)
        assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (name, hex(word))
    for d, s, dp, sp, dl, sl in ((4, 0, 0, 0, 0, 0), (0, 4, 0, 0, 0, 0), (0, 0, 4, 0, 0, 0), (0, 0, 0, 4, 0, 0), (0, 0, 0, 0, 4, 0), (0, 0, 0, 0, 0, 4)):
        rc = lib.cvttmi_resize_image_device(gpu_ctx._h, dst.data_ptr() + d, dw - 1, dh - 1, (dw - 1) * 8 + dp, (dw - 1) * 8 * (dh - 1) + 8 + dl,
                                            src.data_ptr() + s, w - 1, h - 1, (w - 1) * 8 + sp, (w - 1) * 8 * (h - 1) + 8 + sl, HALF, 1, ok,
                                            rwork.data_ptr(), work_bytes + 4096, stream)
        assert rc == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), (d, s, dp, sp, dl, sl)
    check_dst.untouched()
    check_rwork.untouched()
    unchanged()
    image = _cuda(_random(w, h))
    for call in (lambda: gpu_ctx.build_mips(image, kernel="lanczos3"), lambda: gpu_ctx.build_mips(image, hdr="signed"),
                 lambda: gpu_ctx.build_mips(image, kernel="lanczos3", hdr="both"), lambda: gpu_ctx.build_mips(image, filter="normal", kernel="kaiser", hdr="signed"),
                 lambda: gpu_ctx.build_mips(torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda"), kernel="kaiser", hdr="signed"),
                 lambda: gpu_ctx.encode_mips("bc1", torch.zeros((8, 8, 4), dtype=torch.uint8, device="cuda"), kernel="kaiser", hdr="nonnegative")):
        with pytest.raises(api.CvttError):
            call()
    # the 2x2 box of RGBA16F is what it was, flag or no kernel
    assert len(gpu_ctx.build_mips(image)) == 5


# ---- the packer ----

def test_packer_writes_bc6h_files(gpu_ctx, tmp_path, capsys):
    import torch
    bits = _radiance(37, 21, False)
    src = str(tmp_path / "src.npy")
    np.save(src, bits.view(np.float16))
    out = str(tmp_path / "out.dds")
    assert packer.main(["-format", "bc6hu", "-mipkernel", "kaiser", "-dds", "-metrics", src, out]) == 0
    name, w, h, levels = container.read_dds_mips(out)
    assert (name, w, h, len(levels)) == ("bc6hu", 37, 21, 6)
    want = gpu_ctx.encode_mips("bc6hu", _cuda(bits), kernel="kaiser", hdr="nonnegative")
    assert all((a == b.cpu().numpy()).all() for a, b in zip(levels, want))
    assert [l.split()[:3] for l in capsys.readouterr().out.strip().split("\n") if l.startswith("mip ")][:2] == [["mip", "1", "18x10"], ["mip", "2", "9x5"]]
    # signed, from float32, resized first
    signed = _radiance(37, 21, True).view(np.float16)
    np.save(src, signed.astype(np.float32))
    out = str(tmp_path / "out.ktx")
    assert packer.main(["-format", "bc6hs", "-resize", "20x12", "-mips", src, out]) == 0
    name, w, h, levels = container.read_ktx_mips(out)
    assert (name, w, h, len(levels)) == ("bc6hs", 20, 12, 5)
    small = gpu_ctx.resize(_cuda(signed.view(np.uint16)), 20, 12, hdr="signed")
    assert (_bits(small) == ref.resize(signed.view(np.uint16), 20, 12, "lanczos3", "signed")).all()
    want = gpu_ctx.encode_mips("bc6hs", small)
    assert all((a == b.cpu().numpy()).all() for a, b in zip(levels, want))
    # the unpacker on one level: the image decode_image gives for that level's blocks
    image = str(tmp_path / "level1.npy")
    assert unpacker.main(["-level", "1", out, image]) == 0
    decoded = gpu_ctx.decode_image("bc6hs", torch.from_numpy(levels[1].copy()).cuda(), 10, 6)
    assert (np.load(image).view(np.uint16) == _bits(decoded)).all()
    capsys.readouterr()
