"""Decode every format and measure the encoding error in one pass (include/cvtt_mi355x.h, "every format").

CPU: the numpy restatement (texture_decode_ref.py) against Pillow's DDS decoder (tests/golden/bcn_pillow.npz), the coverage
of the seeded random blocks the GPU tests use, the cvttmi_error_totals layout and cvttmi_psnr.
GPU: every decoder against the restatement, host and device forms, the measure's per-block values and totals (exact; BC6H
in the documented float order), determinism across streams, the image form, error codes and the packer's -metrics.
The restatement's own independent anchor is tests/test_encoder_error_anchor.py: the final per-block error of the encoder."""
import ctypes
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import texture_decode_ref as R
from block_fields import etc_modes as _etc_modes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW_FORMATS = ["bc1", "bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s", "etc1", "etc2", "etc2rgba", "etc2punchthrough", "eac",
               "r11u", "r11s"]


def random_blocks(fmt, n=4096, seed=0):
    bpb = R.FORMATS[fmt][1]
    rng = np.random.Generator(np.random.PCG64(1000 + R.FORMATS[fmt][0] + 97 * seed))
    return rng.integers(0, 256, (n, bpb), dtype=np.uint8)


def random_source(fmt, n, seed=0):
    rng = np.random.Generator(np.random.PCG64(5000 + R.FORMATS[fmt][0] + 97 * seed))
    if fmt in ("bc6hu", "bc6hs"):
        lo = -2.0 if fmt == "bc6hs" else 0.0
        return rng.uniform(lo, 4.0, (n, 16, 4)).astype(np.float16).view(np.int16)
    if fmt in ("r11u", "r11s"):
        return rng.integers(-1200, 2200, (n, 16), dtype=np.int16)  # outside the encoder's range too: it clamps
    return rng.integers(0, 256, (n, 16, 4), dtype=np.uint8)


def golden_sets():
    """(fmt, packed, source) of every reference-encoded golden"""
    bc1 = np.load(os.path.join(GOLD, "bc1_mixed.npz"))
    s3 = np.load(os.path.join(GOLD, "s3tc_mixed.npz"))
    etc = np.load(os.path.join(GOLD, "etc2_mixed.npz"))
    ka = np.load(os.path.join(GOLD, "known_answers.npz"))
    out = [("bc1", bc1["out_" + name], bc1["blocks"]) for name in bc1["names"]]
    for key in s3.files:
        if key.startswith("out_"):
            fmt = key.split("_")[1]
            out.append((fmt, s3[key], s3["blocks"].view(np.int8) if fmt.endswith("s") else s3["blocks"]))
    for key in etc.files:
        for prefix, fmt in (("out_rgb_", "etc2"), ("out_rgba_", "etc2rgba"), ("out_alpha_", "eac"), ("out_etc1_", "etc1")):
            if key.startswith(prefix):
                out.append((fmt, etc[key], etc["blocks"]))
        if key.startswith("pt_out_"):
            out.append(("etc2punchthrough", etc[key], etc["pt_blocks"]))
    out.append(("r11u", etc["r11_unsigned"], etc["r11_blocks"]))
    out.append(("r11s", etc["r11_signed"], etc["r11_blocks"]))
    out.append(("bc1", ka["bc1"], ka["blocks"]))
    out.append(("etc2rgba", ka["etc2rgba"], ka["blocks"]))
    return out


# ---------------------------------------------------------------- CPU

def test_numpy_restatement_against_pillow():
    """within 1 of Pillow's DDS decoder; exact on endpoint, transparent and BC2-alpha texels.  BC5S: Pillow stores v + 128
    and does not read -128 as -127 like the reference, so blocks with a -128 endpoint may differ by 2."""
    g = np.load(os.path.join(GOLD, "bcn_pillow.npz"))
    for fmt in ("bc1", "bc2", "bc3", "bc4u", "bc5u", "bc5s"):
        bc, pil = g[fmt + "_bc"], g[fmt + "_rgba"].astype(int)
        d = R.decode(fmt, bc).astype(int)
        if fmt == "bc4u":
            ours, chans = np.stack([d[:, :, 0]] * 3 + [np.full_like(d[:, :, 0], 255)], -1), [0, 1, 2, 3]
        elif fmt in ("bc5u", "bc5s"):
            ours, chans = d + (128 if fmt == "bc5s" else 0), [0, 1]
        else:
            ours, chans = d, [0, 1, 2, 3]
        diff = np.abs(ours - pil)[:, :, chans]
        if fmt == "bc5s":
            minus128 = ((bc[:, [0, 1, 8, 9]] == 128).any(axis=1))
            assert diff[minus128].max() <= 2
            diff = diff[~minus128]
            bc = bc[~minus128]
        assert diff.max() <= 1, fmt
        # endpoint texels (and BC1 transparent texels) exactly
        if fmt in ("bc1", "bc2", "bc3"):
            off = 0 if fmt == "bc1" else 8
            idx = (R._u32(bc, off + 4)[:, None] >> (2 * np.arange(16))) & 3
            c0, c1 = R._u16(bc, off), R._u16(bc, off + 2)
            four = (c0 > c1)[:, None] | (fmt != "bc1")
            exact = (idx <= 1) | (~four & (idx == 3))
            assert (diff[:, :, :3].max(axis=2)[exact] == 0).all(), fmt
        if fmt == "bc2":
            assert (diff[:, :, 3] == 0).all()
        for ch_off, ch in ((0, 3 if fmt == "bc3" else 0), (8, 1)):
            if fmt in ("bc3", "bc4u", "bc5u", "bc5s") and not (ch_off == 8 and fmt in ("bc3", "bc4u")):
                bits = sum(bc[:, ch_off + 2 + i].astype(np.int64) << (8 * i) for i in range(6))
                idx = (bits[:, None] >> (3 * np.arange(16))) & 7
                e0 = bc[:, ch_off].astype(np.int8 if fmt == "bc5s" else np.uint8).astype(int)
                e1 = bc[:, ch_off + 1].astype(np.int8 if fmt == "bc5s" else np.uint8).astype(int)
                six = (e0 <= e1)[:, None]
                # (six-level index 6 of a signed block is -1.0: the reference reads it as -127, Pillow as -128)
                exact = (idx <= 1) | (six & (idx >= (7 if fmt == "bc5s" else 6)))
                assert (diff[:, :, chans.index(ch) if fmt.startswith("bc5") else ch][exact] == 0).all(), fmt


def test_random_fixtures_cover_every_mode():
    """the seeded random blocks of the GPU tests reach every mode the decoders distinguish"""
    b = random_blocks("bc1")
    assert ((R._u16(b, 0) > R._u16(b, 2)).sum() > 100) and ((R._u16(b, 0) <= R._u16(b, 2)).sum() > 100)
    for fmt in ("bc4u", "bc4s", "bc5u", "bc5s"):
        b = random_blocks(fmt)
        a0, a1 = b[:, 0].astype(np.int8 if fmt.endswith("s") else np.uint8), b[:, 1].astype(np.int8 if fmt.endswith("s") else np.uint8)
        assert (a0 > a1).sum() > 100 and (a0 <= a1).sum() > 100
        if fmt.endswith("s"):
            assert (b[:, :2] == 128).any(axis=1).sum() > 5  # signed -128 endpoints
    for fmt, pt in (("etc2", False), ("etc1", False), ("etc2punchthrough", True)):
        modes = _etc_modes(random_blocks(fmt), punchthrough=pt)
        for name, m in modes.items():
            if name == "individual" and pt or name == "opaque0" and not pt:
                continue
            assert m.sum() > 20, (fmt, name)
    modes = _etc_modes(random_blocks("etc2rgba"), 8)
    assert all(m.sum() > 20 for k, m in modes.items() if k != "opaque0")


def test_error_totals_layout():
    """sizeof(cvttmi_error_totals) and its field offsets, as a C compiler sees the header, equal api.ErrorTotals"""
    from convectionkernels_amd import api
    import tempfile
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"cvtt_mi355x.h\"\nint main(void){printf(\"%zu %zu %zu %zu %zu %zu\\n\","
           "sizeof(cvttmi_error_totals), offsetof(cvttmi_error_totals, sse), offsetof(cvttmi_error_totals, sseHdr),"
           "offsetof(cvttmi_error_totals, texels), offsetof(cvttmi_error_totals, channelMask), offsetof(cvttmi_error_totals, format));"
           "return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        with open(c, "w") as f:
            f.write(src)
        subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    T = api.ErrorTotals
    assert got == [80, 0, 32, 64, 72, 76]
    assert got == [ctypes.sizeof(T), T.sse.offset, T.sseHdr.offset, T.texels.offset, T.channelMask.offset, T.format.offset]


def test_psnr_arithmetic():
    from convectionkernels_amd import api
    for fmt in ("bc1", "bc4s", "bc5s", "r11u", "r11s", "etc2", "eac", "bc5u"):
        fid, _, mask, peak = R.FORMATS[fmt]
        t = api.ErrorTotals()
        t.format, t.channelMask, t.texels = fid, mask, 4096
        sse = [1234, 5678, 91011, 1213]
        for c in range(4):
            t.sse[c] = sse[c] if (mask >> c) & 1 else 0
        n = bin(mask).count("1")
        total = sum(t.sse[c] for c in range(4))
        expect = 10.0 * np.log10(peak * peak / (total / (4096.0 * n)))
        assert api.psnr_of_totals(t) == pytest.approx(expect, rel=1e-12), fmt
        assert api.psnr_of_totals(t) == pytest.approx(R.psnr(fmt, list(t.sse), 4096), rel=1e-12)
        assert np.isnan(api.psnr_of_totals(t, 0xF & ~mask or 0x10))  # channels the format does not store
        for c in range(4):
            t.sse[c] = 0
        assert api.psnr_of_totals(t) == float("inf")
    t = api.ErrorTotals()
    t.format, t.channelMask, t.texels = 2, 0x7, 16
    t.sseHdr[0] = 1.0
    assert np.isnan(api.psnr_of_totals(t))  # BC6H: MSE only
    t.format = 3
    assert np.isnan(api.psnr_of_totals(t))
    t.format = 99
    assert np.isnan(api.psnr_of_totals(t))


def test_device_order_restatement_sums_everything():
    """the numpy restatement of the device's float64 reduction adds every block once, across launches too"""
    x = np.arange(1, 5000 * 4 + 1, dtype=np.float64).reshape(-1, 4).astype(np.float32)
    assert (R.device_total(x) == x.astype(np.float64).sum(axis=0)).all()
    assert (R.device_total(x, launch=1 << 12) == x.astype(np.float64).sum(axis=0)).all()


# ---------------------------------------------------------------- GPU

def _numpy_decoded(gpu_ctx, fmt, packed):
    """the restatement's decode; BC7 / BC6H through the existing decoders (tests/test_decode.py holds them to the reference)"""
    if fmt not in ("bc7", "bc6hu", "bc6hs"):
        return R.decode(fmt, packed)
    n = len(packed)
    padded = np.concatenate([packed, np.zeros(((-n) % 8, 16), np.uint8)])
    dec = gpu_ctx.decode_bc7(padded) if fmt == "bc7" else gpu_ctx.decode_bc6h(padded, signed=(fmt == "bc6hs"))
    return dec[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", NEW_FORMATS)
def test_decoders_match_restatement(gpu_ctx, fmt):
    import torch
    sets = [p for f, p, _ in golden_sets() if f == fmt] + [random_blocks(fmt)]
    for packed in sets:
        packed = np.ascontiguousarray(packed)
        packed = packed[: len(packed) // 8 * 8]
        exp = R.decode(fmt, packed)
        host = gpu_ctx.decode(fmt, packed)
        assert host.dtype == exp.dtype and host.shape == exp.shape
        assert (host == exp).all(), fmt
        dev = gpu_ctx.decode(fmt, torch.from_numpy(packed).cuda()).cpu().numpy()
        assert (dev == exp).all(), fmt


@pytest.mark.gpu
def test_decode_bc7_bc6h_unchanged(gpu_ctx):
    """decode("bc7") / decode_bc7 and decode("bc6h*") / decode_bc6h are two spellings of one C entry: each is held to the
    reference's own output (tests/golden/decode.npz), not to the other; on random bytes they still agree"""
    g = np.load(os.path.join(GOLD, "decode.npz"))
    rnd = random_blocks("bc7")
    for fmt, key, named in _BC67_SPELLINGS:
        for spelling in (lambda p: gpu_ctx.decode(fmt, p), lambda p: named(gpu_ctx, p)):
            assert (spelling(g[key + "_in"]) == g[key + "_out"]).all(), fmt
        assert (gpu_ctx.decode(fmt, rnd) == named(gpu_ctx, rnd)).all(), fmt


_BC67_SPELLINGS = (("bc7", "bc7", lambda ctx, p: ctx.decode_bc7(p)),
                   ("bc6hu", "bc6u", lambda ctx, p: ctx.decode_bc6h(p, signed=False)),
                   ("bc6hs", "bc6s", lambda ctx, p: ctx.decode_bc6h(p, signed=True)))


@pytest.mark.gpu
def test_decode_bc7_bc6h_spellings_vs_reference_on_this_box(gpu_ctx, ref_lib):
    """random bytes (every mode, reserved ids): both spellings against the reference's decoders, as tests/test_decode.py"""
    rnd = random_blocks("bc7")
    exp = {"bc7": ref_lib.decode_bc7(rnd), "bc6hu": ref_lib.decode_bc6h(rnd, False), "bc6hs": ref_lib.decode_bc6h(rnd, True)}
    for fmt, _, named in _BC67_SPELLINGS:
        assert (gpu_ctx.decode(fmt, rnd) == exp[fmt]).all(), fmt
        assert (named(gpu_ctx, rnd) == exp[fmt]).all(), fmt


def _measure_cases():
    cases = [(f, p, s) for f, p, s in golden_sets()]
    b7 = np.load(os.path.join(GOLD, "bc7_mixed.npz"))
    cases += [("bc7", b7["out_" + n], b7["blocks"]) for n in b7["names"]]
    b6 = np.load(os.path.join(GOLD, "bc6h_mixed.npz"))
    cases += [("bc6hu", b6["out_default"], b6["blocks"]), ("bc6hs", b6["outs_default"], b6["blocks_signed"])]
    for fmt in ["bc7", "bc6hu", "bc6hs"] + NEW_FORMATS:
        cases.append((fmt, random_blocks(fmt, 2048, 1), random_source(fmt, 2048, 1)))
    return cases


@pytest.mark.gpu
def test_measure_matches_restatement(gpu_ctx):
    import torch
    for fmt, packed, source in _measure_cases():
        n = len(packed) // 8 * 8
        packed, source = np.ascontiguousarray(packed[:n]), np.ascontiguousarray(source[:n])
        exp, exp_pb = R.measure(fmt, _numpy_decoded(gpu_ctx, fmt, packed), source)
        for rep in (gpu_ctx.measure_error(fmt, source, packed, per_block=True),
                    gpu_ctx.measure_error(fmt, torch.from_numpy(source).cuda(), torch.from_numpy(packed).cuda(), per_block=True)):
            pb = rep.per_block if isinstance(rep.per_block, np.ndarray) else rep.per_block.cpu().numpy()
            assert rep.texels == exp["texels"] == 16 * n
            assert rep.channel_mask == R.FORMATS[fmt][2]
            if fmt in ("bc6hu", "bc6hs"):
                # (the golden sources hold infinite halves: such a block is NaN, whatever NaN's bit pattern)
                assert np.array_equal(pb, exp_pb, equal_nan=True), fmt
                assert np.array_equal(np.array(rep.totals.sseHdr), np.array(exp["sse_hdr"]), equal_nan=True), fmt
                assert list(rep.totals.sse) == [0, 0, 0, 0]
            else:
                assert (pb.astype(np.uint32) == exp_pb).all(), fmt
                assert list(rep.totals.sse) == exp["sse"], fmt


@pytest.mark.gpu
def test_measure_matches_reference_decoder(gpu_ctx, ref_lib):
    """BC7 / BC6H: the fused measure's SSE equals that of the reference's own decoder"""
    b7 = np.load(os.path.join(GOLD, "bc7_mixed.npz"))
    packed = np.concatenate([b7["out_default"], random_blocks("bc7", 512, 2)])
    src = np.concatenate([b7["blocks"], random_source("bc7", 512, 2)])
    d = ref_lib.decode_bc7(packed).astype(np.int64) - src.astype(np.int64)
    rep = gpu_ctx.measure_error("bc7", src, packed)
    assert list(rep.totals.sse) == [int(v) for v in (d * d).sum(axis=(0, 1))]
    for fmt in ("bc6hu", "bc6hs"):
        packed, src = random_blocks(fmt, 512, 3), random_source(fmt, 512, 3)
        dec = ref_lib.decode_bc6h(packed, fmt == "bc6hs")
        exp = R.measure(fmt, dec, src)[0]
        rep = gpu_ctx.measure_error(fmt, src, packed)
        assert [float(v) for v in rep.totals.sseHdr] == [float(v) for v in exp["sse_hdr"]]


@pytest.mark.gpu
def test_measure_deterministic_across_streams(gpu_ctx):
    import torch
    n = 1 << 16
    for fmt in ("bc6hu", "bc1", "bc7"):
        packed = torch.from_numpy(random_blocks(fmt, n, 4)).cuda()
        src = torch.from_numpy(random_source(fmt, n, 4)).cuda()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        a = gpu_ctx.measure_error(fmt, src, packed, stream=s1.cuda_stream)
        b = gpu_ctx.measure_error(fmt, src, packed, stream=s2.cuda_stream)
        assert bytes(a.totals) == bytes(b.totals), fmt
        if fmt == "bc6hu":
            exp = R.measure(fmt, gpu_ctx.decode_bc6h(packed.cpu().numpy()), src.cpu().numpy())[0]
            assert [float(v) for v in a.totals.sseHdr] == [float(v) for v in exp["sse_hdr"]]


@pytest.mark.gpu
def test_measure_psnr_agrees_with_psnr_bc7(gpu_ctx):
    import torch
    from convectionkernels_amd import synth
    t = torch.from_numpy(synth.tile_blocks(synth.image_rgba8(2, 256, 256))).cuda()
    packed = gpu_ctx.encode_bc7(t)
    assert abs(gpu_ctx.measure_error("bc7", t, packed).psnr() - gpu_ctx.psnr_bc7(t, packed)) < 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(37, 23), (4096, 4096), (64, 32)])
def test_measure_image(gpu_ctx, size):
    import torch
    from convectionkernels_amd import synth
    w, h = size
    rng = np.random.Generator(np.random.PCG64(w * 7 + h))
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 3) & 255, (y * 5) & 255, (x + y) & 255, 255 - (x & 127)], -1).astype(np.uint8)
    img ^= rng.integers(0, 16, img.shape, dtype=np.uint8)  # some texture
    dev = torch.from_numpy(img).cuda()
    blocks, valid = R.image_to_blocks(img, "bc1")
    fmts = ["bc1", "bc3", "bc4s", "bc5u", "etc2", "etc2punchthrough", "eac", "bc7"] if w < 1000 else ["bc1", "etc2rgba", "bc7"]
    for fmt in fmts:
        packed = gpu_ctx.encode_image(fmt, dev)
        rep = gpu_ctx.measure_image(fmt, dev, packed, per_block=True)
        pk = packed.cpu().numpy()
        src = blocks.view(np.int8) if fmt in ("bc4s", "bc5s") else blocks
        exp, exp_pb = R.measure(fmt, _numpy_decoded(gpu_ctx, fmt, pk), src, valid)
        assert rep.texels == w * h
        assert list(rep.totals.sse) == exp["sse"], fmt
        assert (rep.per_block.cpu().numpy().astype(np.uint32) == exp_pb).all(), fmt
        if w % 32 == 0 and h % 4 == 0:
            tiles = gpu_ctx.tile_image(dev)
            blk = gpu_ctx.measure_error(fmt, tiles.view(torch.int8) if fmt in ("bc4s", "bc5s") else tiles, packed)
            assert bytes(blk.totals) == bytes(rep.totals), fmt
    # BC6H from an RGBA16F image (8-byte texels): against the restatement, float order included, and the block form
    hdr_np = np.ascontiguousarray((img.astype(np.float32) / 64.0).astype(np.float16).view(np.int16))
    hdr = torch.from_numpy(hdr_np).cuda()
    hblocks, hvalid = R.image_to_blocks(hdr_np, "bc6hu")
    for fmt in (("bc6hu", "bc6hs") if w < 1000 else ("bc6hu",)):
        packed = gpu_ctx.encode_image(fmt, hdr)
        rep = gpu_ctx.measure_image(fmt, hdr, packed, per_block=True)
        exp, exp_pb = R.measure(fmt, _numpy_decoded(gpu_ctx, fmt, packed.cpu().numpy()), hblocks, hvalid)
        assert rep.texels == w * h
        assert (rep.per_block.cpu().numpy().view(np.uint32) == exp_pb.view(np.uint32)).all(), fmt
        assert [float(v) for v in rep.totals.sseHdr] == [float(v) for v in exp["sse_hdr"]], fmt
        if w % 32 == 0 and h % 4 == 0:
            blk = gpu_ctx.measure_error(fmt, gpu_ctx.tile_image(hdr), packed)
            assert bytes(blk.totals) == bytes(rep.totals), fmt


@pytest.mark.gpu
def test_measure_accumulates_across_launches_and_chunks(gpu_ctx):
    """The paths that add partial totals: a device call of 2^24 + 4096 blocks (two launches, the second adding into the
    totals; 65 536 partials in the first launch's total pass, BC6H's float64 order across all of it), an image whose
    launch boundary falls inside a block row, with a clipped last block column and a row pitch wider than the image, and
    host calls over several 2^17-block chunks."""
    import torch
    base_n, reps = 4096, 4097
    n = base_n * reps
    assert n > 1 << 24
    for fmt in ("r11u", "bc6hu"):
        pk, src = random_blocks(fmt, base_n, 5), random_source(fmt, base_n, 5)
        per_ch, per_block = R.block_channel_sse(fmt, _numpy_decoded(gpu_ctx, fmt, pk), src)
        dpk = torch.from_numpy(pk).cuda().repeat(reps, 1)
        dsrc = torch.from_numpy(src).cuda().repeat((reps,) + (1,) * (src.ndim - 1))
        rep = gpu_ctx.measure_error(fmt, dsrc, dpk, per_block=True)
        assert rep.texels == 16 * n
        pb = rep.per_block.cpu().numpy()
        if fmt == "bc6hu":
            assert (pb.view(np.uint32) == np.tile(per_block, reps).view(np.uint32)).all()
            exp = R.device_total(np.tile(per_ch, (reps, 1)))
            assert [float(v) for v in rep.totals.sseHdr] == [float(v) for v in exp]
        else:
            assert (pb.astype(np.uint32) == np.tile(per_block, reps)).all()
            assert list(rep.totals.sse) == [int(v) * reps for v in per_ch.sum(axis=0)]
        del dpk, dsrc, rep
        torch.cuda.empty_cache()

    # EAC image of 4097 x 4096 blocks, 16387 texels wide (the last block column has 3): block b = base block b % 4096, so
    # the blocks of the last column (bx = 4096) are base blocks by
    fmt, bw, bh, width = "eac", 4097, 4096, 16387
    pk, src = random_blocks(fmt, base_n, 6), random_source(fmt, base_n, 6)
    d = R.decode(fmt, pk).astype(np.int64)[:, :, 3] - src.astype(np.int64)[:, :, 3]
    tex = d * d  # (4096, 16) per-texel error of the base blocks
    col3 = tex[:, [3, 7, 11, 15]].sum(axis=1)
    exp_pb = np.tile(tex.sum(axis=1), reps)
    exp_pb[np.arange(bh) * bw + (bw - 1)] -= col3[np.arange(bh)]
    full = torch.from_numpy(src).cuda().repeat(reps, 1, 1).view(bh, bw, 4, 4, 4).permute(0, 2, 1, 3, 4).reshape(bh * 4, bw * 4, 4)
    image = full[:, :width]
    assert image.stride(0) == bw * 16 and image.shape[1] == width
    rep = gpu_ctx.measure_image(fmt, image, torch.from_numpy(pk).cuda().repeat(reps, 1), per_block=True)
    assert rep.texels == width * bh * 4
    assert (rep.per_block.cpu().numpy().astype(np.int64) == exp_pb).all()
    assert list(rep.totals.sse) == [0, 0, 0, int(exp_pb.sum())]
    del full, image, rep
    torch.cuda.empty_cache()

    # host entry, three chunks and a bit: chunk totals added on the host in order
    n = 3 * (1 << 17) + 8
    for fmt in ("bc6hs", "bc1"):
        pk, src = random_blocks(fmt, n, 7), random_source(fmt, n, 7)
        rep = gpu_ctx.measure_error(fmt, src, pk, per_block=True)
        per_ch, per_block = R.block_channel_sse(fmt, _numpy_decoded(gpu_ctx, fmt, pk), src)
        assert rep.texels == 16 * n
        if fmt == "bc6hs":
            assert (rep.per_block.view(np.uint32) == per_block.view(np.uint32)).all()
            exp = R.device_total(per_ch, launch=1 << 17)
            assert [float(v) for v in rep.totals.sseHdr] == [float(v) for v in exp]
        else:
            assert (rep.per_block == per_block).all()
            assert list(rep.totals.sse) == [int(v) for v in per_ch.sum(axis=0)]


@pytest.mark.gpu
def test_error_codes(gpu_ctx):
    import torch
    from convectionkernels_amd import api
    lib, h = gpu_ctx._lib, gpu_ctx._h
    packed = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    src = torch.zeros((16, 16, 4), dtype=torch.uint8, device="cuda")
    tot = torch.zeros(80, dtype=torch.uint8, device="cuda")
    out = torch.zeros((16, 64), dtype=torch.uint8, device="cuda")
    E = -1
    for bad in (-1, 17, 1000):
        assert lib.cvttmi_decode_device(h, bad, out.data_ptr(), packed.data_ptr(), 8, None) == E
        assert lib.cvttmi_measure_error_device(h, bad, packed.data_ptr(), src.data_ptr(), 8, None, tot.data_ptr(), None) == E
        assert lib.cvttmi_measure_image_error_device(h, bad, packed.data_ptr(), src.data_ptr(), 8, 8, 32, 0, None, tot.data_ptr(), None) == E
    assert lib.cvttmi_decode_device(h, 1, out.data_ptr(), packed.data_ptr(), 12, None) == E
    assert lib.cvttmi_measure_error_device(h, 1, packed.data_ptr(), src.data_ptr(), 12, None, tot.data_ptr(), None) == E
    assert lib.cvttmi_decode_device(h, 1, None, packed.data_ptr(), 8, None) == E
    assert lib.cvttmi_decode_device(h, 1, out.data_ptr(), None, 8, None) == E
    assert lib.cvttmi_measure_error_device(h, 1, None, src.data_ptr(), 8, None, tot.data_ptr(), None) == E
    assert lib.cvttmi_measure_error_device(h, 1, packed.data_ptr(), None, 8, None, tot.data_ptr(), None) == E
    assert lib.cvttmi_measure_error_device(h, 1, packed.data_ptr(), src.data_ptr(), 8, None, None, None) == E
    host_out = np.zeros((16, 64), np.uint8)
    assert lib.cvttmi_decode(h, 1, host_out.ctypes.data, None, 8) == E
    t = api.ErrorTotals()
    assert lib.cvttmi_measure_error(h, 1, None, host_out.ctypes.data, 8, None, ctypes.addressof(t)) == E
    assert lib.cvttmi_measure_error(h, 1, host_out.ctypes.data, host_out.ctypes.data, 8, None, None) == E
    assert lib.cvttmi_measure_error(h, 1, host_out.ctypes.data, host_out.ctypes.data, 9, None, ctypes.addressof(t)) == E
    # image form: format / pixel kind pairs it does not support (R11; BC6H from RGBA8; RGBA8 formats from RGBA16F)
    for fmt, pixels in ((15, 0), (16, 0), (2, 0), (1, 1), (15, 1)):
        assert lib.cvttmi_measure_image_error_device(h, fmt, packed.data_ptr(), src.data_ptr(), 8, 8, 64, pixels, None,
                                                     tot.data_ptr(), None) == E
    assert lib.cvttmi_measure_image_error_device(h, 1, packed.data_ptr(), src.data_ptr(), 8, 8, 16, 0, None, tot.data_ptr(), None) == E
    # the multi-device entries take every id of the table (each shard is one cvttmi_encode call) and refuse any other
    m = ctypes.c_void_p()
    devs = (ctypes.c_int * 1)(0)
    assert lib.cvttmi_multi_create(ctypes.byref(m), devs, 1) == 0
    try:
        blocks = np.zeros((8, 16, 4), np.uint8)
        o = np.zeros((8, 16), np.uint8)
        opt = api.Options()
        for fid in range(6, 17):
            assert lib.cvttmi_multi_encode(m, fid, o.ctypes.data, blocks.ctypes.data, 8, 0, ctypes.addressof(opt), None) == 0, fid
        for bad in (-1, 17, 1000):
            assert lib.cvttmi_multi_encode(m, bad, o.ctypes.data, blocks.ctypes.data, 8, 0, ctypes.addressof(opt), None) == E, bad
        assert lib.cvttmi_multi_encode(m, 0, o.ctypes.data, blocks.ctypes.data, 8, 0, ctypes.addressof(opt), None) == E  # BC7 without a plan
    finally:
        lib.cvttmi_multi_destroy(m)
    # the Python face
    with pytest.raises(api.CvttError):
        gpu_ctx.decode("bc9", np.zeros((8, 16), np.uint8))
    with pytest.raises(api.CvttError):
        gpu_ctx.measure_error("bc1", np.zeros((12, 16, 4), np.uint8), np.zeros((12, 8), np.uint8))


@pytest.mark.gpu
def test_packer_metrics(gpu_ctx, tmp_path):
    import torch
    from convectionkernels_amd import packer
    rng = np.random.Generator(np.random.PCG64(77))
    y, x = np.mgrid[0:40, 0:52]
    img = np.stack([x * 4, y * 6, (x + y) * 2, np.full_like(x, 255)], -1).astype(np.uint8) ^ rng.integers(0, 8, (40, 52, 4), dtype=np.uint8)
    np.save(tmp_path / "in.npy", img)
    for fmt in ("etc2rgb", "bc1", "bc5u"):
        ext = "dds" if fmt.startswith("bc") else "ktx"
        flags = ["-dds"] if ext == "dds" else []
        plain, metr = io.StringIO(), io.StringIO()
        old = sys.stdout
        try:
            sys.stdout = plain
            assert packer.main(["-format", fmt] + flags + [str(tmp_path / "in.npy"), str(tmp_path / ("a." + ext))]) == 0
            sys.stdout = metr
            assert packer.main(["-format", fmt, "-metrics"] + flags + [str(tmp_path / "in.npy"), str(tmp_path / ("b." + ext))]) == 0
        finally:
            sys.stdout = old
        assert plain.getvalue() == ""
        assert (tmp_path / ("a." + ext)).read_bytes() == (tmp_path / ("b." + ext)).read_bytes()
        lines = metr.getvalue().strip().split("\n")
        rep = gpu_ctx.measure_image(fmt if fmt != "etc2rgb" else "etc2", torch.from_numpy(img).cuda(),
                                    gpu_ctx.encode_image(fmt if fmt != "etc2rgb" else "etc2", torch.from_numpy(img).cuda()))
        assert len(lines) == len(rep.channels) + 1
        assert lines[-1].startswith("psnr %.4f dB" % rep.psnr())
