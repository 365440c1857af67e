"""Context.encode(fmt, ...) -- every encoder by its format name -- against the methods named after the reference's calls, and
encode_image through it."""
import numpy as np
import pytest

import content
from convectionkernels_amd import api

# name of TEXTURE_FORMATS -> the named method on a context
NAMED = {
    "bc7": lambda c, b, **kw: c.encode_bc7(b, **kw),
    "bc1": lambda c, b, **kw: c.encode_bc1(b, **kw),
    "bc2": lambda c, b, **kw: c.encode_bc2(b, **kw),
    "bc3": lambda c, b, **kw: c.encode_bc3(b, **kw),
    "bc4u": lambda c, b, **kw: c.encode_bc4(b, signed=False, **kw),
    "bc4s": lambda c, b, **kw: c.encode_bc4(b, signed=True, **kw),
    "bc5u": lambda c, b, **kw: c.encode_bc5(b, signed=False, **kw),
    "bc5s": lambda c, b, **kw: c.encode_bc5(b, signed=True, **kw),
    "bc6hu": lambda c, b, **kw: c.encode_bc6h(b, signed=False, **kw),
    "bc6hs": lambda c, b, **kw: c.encode_bc6h(b, signed=True, **kw),
    "etc1": lambda c, b, **kw: c.encode_etc1(b, **kw),
    "etc2": lambda c, b, **kw: c.encode_etc2(b, **kw),
    "etc2rgb": lambda c, b, **kw: c.encode_etc2(b, **kw),
    "etc2rgba": lambda c, b, **kw: c.encode_etc2_rgba(b, **kw),
    "etc2punchthrough": lambda c, b, **kw: c.encode_etc2_punchthrough_alpha(b, **kw),
    "eac": lambda c, b, **kw: c.encode_etc2_alpha(b, **kw),
    "r11u": lambda c, b, **kw: c.encode_etc2_alpha11(b, signed=False, **kw),
    "r11s": lambda c, b, **kw: c.encode_etc2_alpha11(b, signed=True, **kw),
}
N = 24


def _source(fmt):
    if fmt in ("bc6hu", "bc6hs"):
        return content.mixed_hdr_blocks(31, N // 8, signed=(fmt == "bc6hs"))[:N]
    if fmt in ("r11u", "r11s"):
        return content.mixed_r11_blocks(32, N // 8)[:N]
    if fmt == "etc2punchthrough":
        return content.punchthrough_blocks(33, 1)[:N]
    b = content.mixed_ldr_blocks(34, N // 8)[:N]
    return b.view(np.int8) if fmt in ("bc4s", "bc5s") else b


def test_every_format_name_has_a_named_method():
    assert set(NAMED) == set(api.TEXTURE_FORMATS)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", list(NAMED))
def test_encode_by_name_equals_the_named_method(gpu_ctx, fmt):
    import torch
    blocks = np.ascontiguousarray(_source(fmt))
    _, out_bytes, in_bytes, _ = api.TEXTURE_FORMATS[fmt]
    assert blocks.nbytes == N * in_bytes
    opt = api.Options()
    named = NAMED[fmt](gpu_ctx, blocks, options=opt)
    assert named.shape == (N, out_bytes) and named.dtype == np.uint8
    assert (gpu_ctx.encode(fmt, blocks, opt) == named).all()
    t = torch.from_numpy(blocks).cuda()
    on_device = gpu_ctx.encode(fmt, t, opt)
    assert on_device.is_cuda and (on_device.cpu().numpy() == named).all()
    assert (NAMED[fmt](gpu_ctx, t, options=opt).cpu().numpy() == named).all()
    if fmt in ("etc2", "etc2rgba", "etc2punchthrough"):  # the Options of AllocETC2Data reach the encoder by both routes
        data = api.AllocETC2Data(api.Options(redWeight=1.0, greenWeight=0.5, blueWeight=0.25))
        with_data = NAMED[fmt](gpu_ctx, blocks, options=opt, compression_data=data)
        assert (gpu_ctx.encode(fmt, t, opt, compression_data=data).cpu().numpy() == with_data).all()
    with pytest.raises(api.CvttError):
        gpu_ctx.encode("bc9", blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bc4s", "etc2punchthrough"])
def test_encode_image_dispatches_by_name(gpu_ctx, fmt):
    """37 x 10: ten real blocks in rows of sixteen, a clipped last block row -- tile, the named method, compact_rows"""
    import torch
    w, h = 37, 10
    img = np.random.Generator(np.random.PCG64(4100)).integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[:, ::3, 3] = 0  # transparent texels for the punch-through encoder
    image = torch.from_numpy(img).cuda()
    opt = api.Options()
    tiles = gpu_ctx.tile_image(image)
    assert tiles.shape[0] == 16 * 3
    exp = gpu_ctx.compact_rows(NAMED[fmt](gpu_ctx, tiles, options=opt), w, h)
    got = gpu_ctx.encode_image(fmt, image, opt)
    assert got.shape == (10 * 3, 8) and (got.cpu().numpy() == exp.cpu().numpy()).all()
    with pytest.raises(api.CvttError):
        gpu_ctx.encode_image("r11u", image)
