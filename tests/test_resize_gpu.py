"""Resizing on the GPU: cvttmi_resize_image_device against the numpy restatement (tests/resize_ref.py, fed with the tables
cvttmi_resize_taps returned) byte for byte in guarded buffers -- both paths (one launch through LDS, two launches through the work
space), every kernel, rule, pixel kind and wrap mode; planted footprints; the identity; exactly half against build_mips; layers
through pitched buffers; calls queued back to back; the packer; what the entry point rejects."""
import ctypes
import functools

import numpy as np
import pytest

import guarded
import resize_ref as ref
from convectionkernels_amd import api, container, packer

pytestmark = pytest.mark.gpu

E_INVALID = -1
RGBA8, SNORM = api.PIXELS_RGBA8, api.PIXELS_RGBA8_SNORM
BOX, SRGB, NORMAL = api.MIP_FILTER_BOX, api.MIP_FILTER_SRGB, api.MIP_FILTER_NORMAL
RULE_NAMES = {BOX: "box", SRGB: "srgb", NORMAL: "normal"}
POISON = 0xA5

# source -> destination, width x height.  The six pairs of the float64 test; 300x70 -> 130x150: several workgroups in both
# directions, up in one axis and down in the other; 257x33 -> 8x8: the longest rows, about 200 taps; 1x1 <-> 9x5; 6x700 -> 5x3: 1400
# taps down a column, far more source rows than LDS holds -- two launches under every rule (257x33 -> 8x8 takes two under SRGB and
# NORMAL, one under the plain rule)
SIZES = [((37, 29), (16, 16)), ((16, 16), (37, 29)), ((64, 48), (21, 64)), ((100, 7), (33, 20)), ((5, 3), (64, 64)), ((257, 33), (32, 8)),
         ((300, 70), (130, 150)), ((257, 33), (8, 8)), ((1, 1), (9, 5)), ((9, 5), (1, 1)), ((6, 700), (5, 3))]
# (kernel, rule, kind): all five kernels under the plain rule; Lanczos3 and box under SRGB and NORMAL; int8 under plain and NORMAL
COMBOS = [(k, BOX, RGBA8) for k in ("box", "triangle", "mitchell", "lanczos3", "kaiser")] + \
         [(k, rule, RGBA8) for k in ("lanczos3", "box") for rule in (SRGB, NORMAL)] + \
         [(k, rule, SNORM) for k in ("lanczos3", "box") for rule in (BOX, NORMAL)]


def _id(v):
    return {RGBA8: "rgba8", SNORM: "snorm"}[v[2]] + "-" + RULE_NAMES[v[1]] + "-" + v[0]


def _size_id(v):
    return "%dx%d-%dx%d" % (v[0] + v[1])


@functools.lru_cache(maxsize=None)
def _image(w, h, kind, seed=0):
    img = np.random.default_rng(7 * w + h + 1000 * seed).integers(0, 256, (h, w, 4), dtype=np.uint8).view(np.int8 if kind == SNORM else np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _tables(w, h, dw, dh, kernel):
    """what the C function returned: the restatement below computes with these"""
    return api.resize_taps(w, dw, kernel), api.resize_taps(h, dh, kernel)


def _want(img, dw, dh, kernel, rule, wrap="clamp"):
    h, w = img.shape[:2]
    return ref.resize(img, dw, dh, kernel, rule, wrap, tables=_tables(w, h, dw, dh, kernel))


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _work_bytes(w, h, dw, dh, kind, word, layers=1):
    need = ctypes.c_size_t(0)
    assert api.load_library().cvttmi_resize_work_bytes(w, h, dw, dh, kind, word, layers, ctypes.byref(need)) == 0
    return need.value


def _resize_guarded(gpu_ctx, images, dw, dh, kind, word, src_gap=(0, 0), dst_gap=(0, 0), what=""):
    """the C call on (L, H, W, 4) numpy images through guarded buffers, rows `gap[0]` texels and layers `gap[1]` rows further apart
    than they need be: returns the (L, dh, dw, 4) result after checking that nothing else was written -- the pitch gaps and guards of
    the destination, the guards of the work space, the source"""
    n, h, w = images.shape[:3]
    src_row, dst_row = 4 * (w + src_gap[0]), 4 * (dw + dst_gap[0])
    src_layer, dst_layer = src_row * (h + src_gap[1]), dst_row * (dh + dst_gap[1])
    held = np.full((n, h + src_gap[1], w + src_gap[0], 4), 0x3C, np.uint8)
    held[:, :h, :w] = images.view(np.uint8)
    src, unchanged = guarded.device_input(held)
    dst, check = guarded.device_buffer(n * dst_layer, poison=POISON, what="resized " + what)
    need = _work_bytes(w, h, dw, dh, kind, word, n)
    work, check_work = guarded.device_buffer(need, poison=POISON, what="work space " + what)
    rc = api.load_library().cvttmi_resize_image_device(gpu_ctx._h, dst.data_ptr(), dw, dh, dst_row, dst_layer, src.data_ptr(), w, h, src_row,
                                                       src_layer, kind, n, word, work.data_ptr(), need, _stream())
    assert rc == 0, gpu_ctx._lib.cvttmi_last_error(gpu_ctx._h)
    got = check.payload().reshape(n, dh + dst_gap[1], dw + dst_gap[0], 4)
    expected = np.full_like(got, POISON)
    expected[:, :dh, :dw] = got[:, :dh, :dw]
    check(expected)                     # the guards and every byte outside dw x dh of each layer still hold the poison
    check_work(check_work.payload())    # the guards of the work space
    unchanged()
    return got[:, :dh, :dw].view(images.dtype).copy()


@pytest.mark.parametrize("combo", COMBOS, ids=_id)
@pytest.mark.parametrize("sizes", SIZES, ids=_size_id)
def test_bytes_of_the_restatement(gpu_ctx, sizes, combo):
    (w, h), (dw, dh) = sizes
    kernel, rule, kind = combo
    img = _image(w, h, kind)
    got = _resize_guarded(gpu_ctx, img[None], dw, dh, kind, api.RESIZE_KERNELS[kernel] | rule, what=_size_id(sizes) + " " + _id(combo))[0]
    assert (got == _want(img, dw, dh, kernel, rule)).all()


def test_both_paths_are_among_the_cases():
    """(no device work) the sizes above reach the one-launch and the two-launch path under every rule"""
    for rule in RULE_NAMES.values():
        took = {api.resize_launches(w, h, dw, dh, "lanczos3", rule) for (w, h), (dw, dh) in SIZES}
        assert took == {1, 2}, rule
    assert api.resize_launches(257, 33, 8, 8, "lanczos3", "box") == 1 and api.resize_launches(257, 33, 8, 8, "lanczos3", "srgb") == 2
    assert api.resize_launches(6, 700, 5, 3, "box", "box") == 2 and api.resize_launches(6, 700, 5, 3, "lanczos3", "box", signed=True) == 2


@pytest.mark.parametrize("wrap", ["repeat", "mirror"])
@pytest.mark.parametrize("combo", [("lanczos3", BOX, RGBA8), ("box", BOX, RGBA8), ("kaiser", SRGB, RGBA8), ("mitchell", NORMAL, SNORM)], ids=_id)
@pytest.mark.parametrize("sizes", [((5, 3), (64, 64)), ((9, 5), (1, 1)), ((6, 700), (5, 3))], ids=_size_id)
def test_wrap_modes_where_the_footprint_exceeds_the_image(gpu_ctx, sizes, combo, wrap):
    (w, h), (dw, dh) = sizes
    kernel, rule, kind = combo
    img = _image(w, h, kind, seed=1)
    got = _resize_guarded(gpu_ctx, img[None], dw, dh, kind, api.RESIZE_KERNELS[kernel] | rule | api.MIP_WRAPS[wrap])[0]
    assert (got == _want(img, dw, dh, kernel, rule, wrap)).all()
    if sizes[0] == (9, 5):
        assert (got != _want(img, dw, dh, kernel, rule, "clamp")).any() or kernel == "box"  # (the box never leaves the image)


@pytest.mark.parametrize("sizes", [((64, 40), (32, 20)), ((45, 30), (14, 9)), ((24, 20), (60, 47))], ids=_size_id)
@pytest.mark.parametrize("kernel", ["box", "triangle", "mitchell", "lanczos3", "kaiser"])
def test_planted_footprints(gpu_ctx, kernel, sizes):
    """the largest value under every positive tap and the smallest under every negative one, and the reverse: h and s at their
    extremes, the texel clamped to the end of its range; at exactly half one footprint whose three NORMAL sums are all zero"""
    (w, h), (dw, dh) = sizes
    for kind, dtype in ((RGBA8, np.uint8), (SNORM, np.int8)):
        img, spots = ref.planted_image(kernel, w, h, dw, dh, dtype)
        assert len(spots) >= 2 and (sizes[1] != (32, 20) or len(spots) == 3)
        for rule in (BOX, SRGB, NORMAL) if kind == RGBA8 else (BOX, NORMAL):
            got = _resize_guarded(gpu_ctx, img[None], dw, dh, kind, api.RESIZE_KERNELS[kernel] | rule)[0]
            assert (got == _want(img, dw, dh, kernel, rule)).all(), (kind, rule)
            if rule != NORMAL:
                for x, y, byte in spots[:2]:
                    assert got[y, x].tolist() == [byte] * 4, (kind, rule, x, y)
            elif len(spots) == 3:
                x, y, _ = spots[2]
                assert (got[y, x] == _want(img, dw, dh, kernel, BOX)[y, x]).all(), (kind, x, y)


@pytest.mark.parametrize("kernel", ["box", "triangle", "mitchell", "lanczos3", "kaiser"])
def test_the_same_size_returns_the_image(gpu_ctx, kernel):
    import torch
    for w, h in ((37, 29), (130, 70)):
        image = torch.from_numpy(_image(w, h, RGBA8).copy()).cuda()
        for rule in ("box", "srgb"):
            for wrap in ("clamp", "mirror"):
                assert torch.equal(gpu_ctx.resize(image, w, h, kernel=kernel, filter=rule, wrap=wrap), image), (w, h, rule, wrap)
    signed = torch.from_numpy(_image(37, 29, SNORM).copy()).cuda()
    assert torch.equal(gpu_ctx.resize(signed, 37, 29, kernel=kernel), signed)


@pytest.mark.parametrize("kernel", ["triangle", "mitchell", "lanczos3", "kaiser"])
@pytest.mark.parametrize("w,h", [(64, 48), (34, 18)])
def test_exactly_half_is_build_mips(gpu_ctx, w, h, kernel):
    """the general tables at 2:1 are the mip kernels': level 1 of the chain, byte for byte"""
    import torch
    image = torch.from_numpy(_image(w, h, RGBA8, seed=2).copy()).cuda()
    signed = torch.from_numpy(_image(w, h, SNORM, seed=2).copy()).cuda()
    for rule in ("box", "srgb", "normal"):
        for wrap in ("clamp", "repeat", "mirror"):
            want = gpu_ctx.build_mips(image, levels=2, filter=rule, kernel=kernel, wrap=wrap)[1]
            assert torch.equal(gpu_ctx.resize(image, w // 2, h // 2, kernel=kernel, filter=rule, wrap=wrap), want), (rule, wrap)
            if rule != "srgb":
                want = gpu_ctx.build_mips(signed, levels=2, filter=rule, kernel=kernel, wrap=wrap)[1]
                assert torch.equal(gpu_ctx.resize(signed, w // 2, h // 2, kernel=kernel, filter=rule, wrap=wrap), want), (rule, wrap, "int8")


@pytest.mark.parametrize("combo", [("lanczos3", BOX, RGBA8), ("kaiser", SRGB, RGBA8), ("mitchell", NORMAL, SNORM), ("box", NORMAL, RGBA8)], ids=_id)
@pytest.mark.parametrize("sizes", [((70, 38), (45, 52)), ((20, 300), (33, 9))], ids=_size_id)
def test_layers_through_pitched_buffers(gpu_ctx, sizes, combo):
    """three layers, rows and layers further apart than they need be on both sides (70x38 -> 45x52: one launch; 20x300 -> 33x9: two):
    every byte outside dstW x dstH of each layer and outside the work space untouched; each layer is the single-image call"""
    (w, h), (dw, dh) = sizes
    kernel, rule, kind = combo
    word = api.RESIZE_KERNELS[kernel] | rule | api.MIP_WRAPS["mirror"]
    images = np.stack([_image(w, h, kind, seed=3 + l) for l in range(3)])
    got = _resize_guarded(gpu_ctx, images, dw, dh, kind, word, src_gap=(3, 2), dst_gap=(5, 1))
    for l in range(3):
        single = _resize_guarded(gpu_ctx, images[l: l + 1], dw, dh, kind, word)[0]
        assert (got[l] == single).all() and (single == _want(images[l], dw, dh, kernel, rule, "mirror")).all(), l


def test_python_layers_out_and_views(gpu_ctx):
    import torch
    images = torch.from_numpy(np.stack([_image(40, 24, RGBA8, seed=l) for l in range(2)])).cuda()
    want = [_want(_image(40, 24, RGBA8, seed=l), 13, 31, "kaiser", SRGB, "repeat") for l in range(2)]
    got = gpu_ctx.resize(images, 13, 31, kernel="kaiser", filter="srgb", wrap="repeat")
    assert got.shape == (2, 31, 13, 4) and got.dtype == torch.uint8 and all((got[l].cpu().numpy() == want[l]).all() for l in range(2))
    # a column slice of a wider image in, a slice of a wider allocation out
    wide = torch.zeros((24, 50, 4), dtype=torch.uint8, device="cuda")
    wide[:, 5:45] = images[0]
    store = torch.full((31, 20, 4), 0x5A, dtype=torch.uint8, device="cuda")
    out = store[:, 2:15]
    assert gpu_ctx.resize(wide[:, 5:45], 13, 31, kernel="kaiser", filter="srgb", wrap="repeat", out=out) is out
    assert (out.cpu().numpy() == want[0]).all() and (store[:, :2] == 0x5A).all() and (store[:, 15:] == 0x5A).all()
    for bad in (dict(kernel="cubic"), dict(filter="box+alpha"), dict(wrap="border"), dict(width=0), dict(height=65536),
                dict(out=torch.zeros((31, 13, 4), dtype=torch.int8, device="cuda")), dict(out=torch.zeros((31, 14, 4), dtype=torch.uint8, device="cuda"))):
        with pytest.raises(api.CvttError):
            gpu_ctx.resize(images[0], **dict(dict(width=13, height=31), **bad))
    with pytest.raises(api.CvttError):
        gpu_ctx.resize(images.view(torch.int8), 13, 31, filter="srgb")
    with pytest.raises(api.CvttError):
        gpu_ctx.resize(torch.zeros((4, 4, 4), dtype=torch.float16, device="cuda"), 2, 2)


def test_calls_queued_back_to_back(gpu_ctx):
    """resizes with different tables on one stream, nothing synchronised in between, while the stream is still busy with what was
    queued before them: more of them than the context has table slots, then the first one's arguments again.  All are right."""
    import torch
    jobs = [((37, 29), (16, 16), "lanczos3", "box"), ((64, 48), (21, 64), "kaiser", "srgb"), ((100, 7), (33, 20), "box", "box"),
            ((16, 16), (37, 29), "mitchell", "normal"), ((6, 700), (5, 3), "triangle", "box"), ((257, 33), (32, 8), "lanczos3", "srgb"),
            ((37, 29), (16, 16), "lanczos3", "box")]
    images = [torch.from_numpy(_image(w, h, RGBA8, seed=4).copy()).cuda() for (w, h), _, _, _ in jobs]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(40_000_000)  # (device cycles: the copies of the tables queue up behind it)
        got = [gpu_ctx.resize(image, dw, dh, kernel=kernel, filter=rule) for image, (_, (dw, dh), kernel, rule) in zip(images, jobs)]
    stream.synchronize()
    for result, ((w, h), (dw, dh), kernel, rule) in zip(got, jobs):
        want = _want(_image(w, h, RGBA8, seed=4), dw, dh, kernel, api.RESIZE_RULES[rule])
        assert (result.cpu().numpy() == want).all(), (w, h, dw, dh, kernel, rule)


def test_rejections(gpu_ctx):
    """CVTTMI_E_INVALID with an error text before anything is queued: the destination and the work space keep their poison"""
    lib = api.load_library()
    w, h, dw, dh = 37, 29, 16, 12
    ok = api.MIP_KERNELS["lanczos3"]
    src, unchanged = guarded.device_input(_image(w, h, RGBA8))
    dst, check = guarded.device_buffer(dw * dh * 4 * 2, poison=POISON)
    need = _work_bytes(w, h, dw, dh, RGBA8, ok, 2)
    work, check_work = guarded.device_buffer(need, poison=POISON)
    good = dict(dst=dst.data_ptr(), dw=dw, dh=dh, drow=dw * 4, dlayer=dw * dh * 4, src=src.data_ptr(), w=w, h=h, srow=w * 4, slayer=w * h * 4,
                kind=RGBA8, layers=1, word=ok, work=work.data_ptr(), need=need)

    def call(**change):
        a = dict(good, **change)
        return lib.cvttmi_resize_image_device(gpu_ctx._h, a["dst"], a["dw"], a["dh"], a["drow"], a["dlayer"], a["src"], a["w"], a["h"], a["srow"],
                                              a["slayer"], a["kind"], a["layers"], a["word"], a["work"], a["need"], _stream())
    bad = [dict(dst=None), dict(src=None), dict(work=None), dict(dst=dst.data_ptr() + 2), dict(src=src.data_ptr() + 1), dict(work=work.data_ptr() + 128),
           dict(dw=0), dict(dh=0), dict(w=0), dict(h=0), dict(layers=0), dict(dw=65536, drow=65536 * 4), dict(layers=65536),
           dict(drow=dw * 4 - 4), dict(drow=dw * 4 + 2), dict(srow=w * 4 - 4), dict(srow=w * 4 + 1), dict(dlayer=dw * dh * 4 - 4), dict(dlayer=dw * dh * 4 + 2),
           dict(slayer=w * h * 4 - 4), dict(slayer=w * h * 4 + 3), dict(need=need - 1), dict(need=0), dict(layers=2, need=_work_bytes(w, h, dw, dh, RGBA8, ok, 1) - 1),
           dict(kind=api.PIXELS_RGBA16F), dict(kind=3), dict(kind=SNORM, word=ok | SRGB), dict(word=ok | api.MIP_FILTER_ALPHA_WEIGHTED), dict(word=ok | 3),
           dict(word=0x50), dict(word=0xF0 | NORMAL), dict(word=ok | 0x600), dict(word=0x600), dict(word=ok | 0x800), dict(word=ok | 0x80000000)]
    for change in bad:
        assert call(**change) == E_INVALID and lib.cvttmi_last_error(gpu_ctx._h), change
    check.untouched()
    check_work.untouched()
    unchanged()
    assert call() == 0 and call(word=0) == 0 and call(layers=1, need=need + 1) == 0  # (and the arguments they vary are fine)
    import torch
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _photo(w, h):
    rng = np.random.default_rng(w)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([x * 255 // w, y * 255 // h, (x + y) * 255 // (w + h), 255 - x * 255 // w], -1) + rng.integers(-12, 13, (h, w, 4))
    return np.clip(img, 0, 255).astype(np.uint8)


def test_packer_resizes_before_anything_else(gpu_ctx, tmp_path, capsys):
    import torch
    image = _photo(37, 29)
    src, out = str(tmp_path / "src.npy"), str(tmp_path / "out.ktx")
    np.save(src, image)
    assert packer.main(["-resize", "20x12", "-format", "bc1", src, out]) == 0
    name, w, h, packed = container.read_ktx(out)
    assert (name, w, h) == ("bc1", 20, 12)
    resized = gpu_ctx.resize(torch.from_numpy(image.copy()).cuda(), 20, 12)
    assert (resized.cpu().numpy() == _want(image, 20, 12, "lanczos3", BOX)).all()
    assert (np.asarray(packed).reshape(-1) == gpu_ctx.encode_image("bc1", resized).cpu().numpy().reshape(-1)).all()
    capsys.readouterr()
    # the chain and the metrics follow from 20x12
    assert packer.main(["-resize", "20x12", "-format", "bc1", "-mips", "-metrics", src, out]) == 0
    name, w, h, levels = container.read_ktx_mips(out)
    assert (name, w, h, len(levels)) == ("bc1", 20, 12, 5) and (np.asarray(levels[0]).reshape(-1) == np.asarray(packed).reshape(-1)).all()
    lines = capsys.readouterr().out.strip().split("\n")
    assert [l.split()[:3] for l in lines if l.startswith("mip ")] == [["mip", "1", "10x6"], ["mip", "2", "5x3"], ["mip", "3", "2x1"], ["mip", "4", "1x1"]]
    assert any(l.startswith("psnr ") and "240 texels" in l for l in lines)
    # the other two size flags, the rule and the kernel; layers in one call
    assert packer.main(["-maxsize", "16", "-resizekernel", "box", "-resizerule", "srgb", "-resizewrap", "mirror", "-format", "bc1", src, out]) == 0
    name, w, h, packed = container.read_ktx(out)
    assert (w, h) == (16, 13)
    resized = gpu_ctx.resize(torch.from_numpy(image.copy()).cuda(), 16, 13, kernel="box", filter="srgb", wrap="mirror")
    assert (np.asarray(packed).reshape(-1) == gpu_ctx.encode_image("bc1", resized).cpu().numpy().reshape(-1)).all()
    stack = str(tmp_path / "stack.npy")
    np.save(stack, np.stack([image, image[::-1]]))
    assert packer.main(["-array", "-pow2", "down", "-format", "bc1", stack, out]) == 0
    both = gpu_ctx.resize(torch.from_numpy(np.stack([image, image[::-1]])).cuda(), 32, 16)
    want = packer.encode_file_texture(both.cpu().numpy(), "bc1")
    name, tw, th, layers, cube = container.read_ktx_texture(out)
    assert (name, tw, th, len(layers), cube) == ("bc1", 32, 16, 2, False)
    assert all((np.asarray(layers[l][0]).reshape(-1) == np.asarray(want[l][0]).reshape(-1)).all() for l in range(2))
