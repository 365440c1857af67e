"""Decoders: the HIP DecodeBC7 / DecodeBC6HU / DecodeBC6HS against golden outputs of the
reference's decoders -- encoder output of every golden variant plus random byte patterns (all modes,
reserved modes) -- and an encode -> decode round trip with the error the encoder itself reported."""
import os

import numpy as np
import pytest

import content

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_decode_fixture_covers_every_mode():
    g = np.load(os.path.join(GOLD, "decode.npz"))
    b0 = g["bc7_in"][:, 0].astype(np.int64)
    modes = set((int(b) & -int(b)).bit_length() - 1 if b else 8 for b in b0)
    assert modes == set(range(9))
    m6 = g["bc6u_in"][:, 0]
    ids = set(int(b & 3) if (b & 3) < 2 else int(b & 31) for b in m6)
    assert {0, 1, 2, 6, 10, 14, 18, 22, 26, 30, 3, 7, 11, 15} <= ids and len(ids) > 14  # all 14 modes + reserved ids


@pytest.mark.gpu
def test_decode_matches_reference_goldens(gpu_ctx):
    import torch
    g = np.load(os.path.join(GOLD, "decode.npz"))
    assert (gpu_ctx.decode_bc7(g["bc7_in"]) == g["bc7_out"]).all()
    assert (gpu_ctx.decode_bc7(torch.from_numpy(g["bc7_in"]).cuda()).cpu().numpy() == g["bc7_out"]).all()
    assert (gpu_ctx.decode_bc6h(g["bc6u_in"], signed=False) == g["bc6u_out"]).all()
    assert (gpu_ctx.decode_bc6h(g["bc6s_in"], signed=True) == g["bc6s_out"]).all()
    assert (gpu_ctx.decode_bc6h(torch.from_numpy(g["bc6u_in"]).cuda()).cpu().numpy() == g["bc6u_out"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,key", [("bc7", "bc7"), ("bc6hu", "bc6u"), ("bc6hs", "bc6s")])
def test_decode_kernel_edges(gpu_ctx, fmt, key):
    """The block-decode kernel at the edges of its 256-lane workgroups, host and device entry, every block against the
    reference's output: 8 blocks (the smallest count: one partly filled workgroup), 264 = 256 + 8 (across one workgroup
    boundary into a nearly empty one), and the whole fixture (2 624 / 2 304 / 2 112 blocks: every mode, the reserved ids; a
    last workgroup of 64 lanes for bc7 and bc6hs, nine full workgroups for bc6hu)"""
    import torch
    g = np.load(os.path.join(GOLD, "decode.npz"))
    packed, exp = g[key + "_in"], g[key + "_out"]
    assert len(packed) == {"bc7": 2624, "bc6hu": 2304, "bc6hs": 2112}[fmt]
    for n in (8, 264, len(packed)):
        host = gpu_ctx.decode(fmt, packed[:n])
        assert host.shape == exp[:n].shape and (host == exp[:n]).all(), (fmt, n)
        dev = gpu_ctx.decode(fmt, torch.from_numpy(packed[:n]).cuda()).cpu().numpy()
        assert dev.shape == exp[:n].shape and (dev == exp[:n]).all(), (fmt, n)


@pytest.mark.gpu
def test_decode_vs_reference_on_this_box(gpu_ctx, ref_lib):
    rng = np.random.Generator(np.random.PCG64(99))
    rnd = rng.integers(0, 256, (4096, 16), dtype=np.uint8)
    assert (gpu_ctx.decode_bc7(rnd) == ref_lib.decode_bc7(rnd)).all()
    assert (gpu_ctx.decode_bc6h(rnd, signed=False) == ref_lib.decode_bc6h(rnd, False)).all()
    assert (gpu_ctx.decode_bc6h(rnd, signed=True) == ref_lib.decode_bc6h(rnd, True)).all()


@pytest.mark.gpu
def test_encode_decode_round_trip(gpu_ctx):
    """decode(encode(x)) stays close to x where BC7 can represent x: solid and two-colour blocks within one grey level,
    the heavily weighted green channel of smooth blocks within a few (the default weights let red and blue drift), and the
    PSNR of pure noise at what an 8 bit/pixel format can do"""
    import torch
    from convectionkernels_amd import synth
    blocks = content.mixed_ldr_blocks(123, 48)
    dec = gpu_ctx.decode_bc7(gpu_ctx.encode_bc7(blocks))
    smooth = np.array([g * 8 + b for g in range(48) if g % 12 == 2 for b in range(8)])
    assert np.abs(dec[smooth].astype(int) - blocks[smooth].astype(int))[:, :, 1].max() <= 8
    solid = np.array([g * 8 + b for g in range(48) if g % 12 == 4 for b in range(8)])
    assert np.abs(dec[solid].astype(int) - blocks[solid].astype(int)).max() <= 1
    two = np.array([g * 8 + b for g in range(48) if g % 12 == 5 for b in range(8)])
    assert np.abs(dec[two].astype(int) - blocks[two].astype(int)).max() <= 1
    t = torch.from_numpy(synth.tile_blocks(synth.image_rgba8(2, 512, 512))).cuda()
    psnr = gpu_ctx.psnr_bc7(t, gpu_ctx.encode_bc7(t))
    assert 10.0 < psnr < 30.0
    hdr = content.mixed_hdr_blocks(5, 8)
    dh = gpu_ctx.decode_bc6h(gpu_ctx.encode_bc6h(hdr), signed=False)
    assert dh.shape == hdr.shape and (dh[:, :, 3] == 0x3C00).all()
