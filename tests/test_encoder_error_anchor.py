"""The LDR decoders and the error measure, held to the encoder's own error.

INTEGRATION.md 3a says that the decoders use the model the reference encoder scores its candidates with, "so the measured
error is the error the encoder minimised".  The C oracle (oracle/cvtt_oracle.c, byte-identical to the reference) keeps, per
block, the score of the candidate it finally emits, and hands it out through OracleLib.encode_*_err.  With Flags::Uniform set
and S3TC_Paranoid / S3TC_Exhaustive clear that score is a plain sum of squared integer differences, at most
16 * 3 * 255^2 < 2^24 and therefore exact in binary32.  So it must equal, block by block and with no tolerance, the squared
error of a correct decode of the emitted bytes against the source.

CPU: the numpy restatement (texture_decode_ref.py) against that number -- the independent anchor of the restatement, which
tests/test_decode_formats.py then holds the kernels to.
GPU: Context.decode, Context.measure_error (per block and totals) and Context.measure_image against the same number, the
encoder's bytes being the oracle's, with no restatement in between.

What is compared, per format (N = 1024 blocks of content.mixed_ldr_blocks, a fixed reciprocal table):
  ETC2 RGB, ETC1          colour error = RGB SSE
  ETC2 punch-through      colour error = RGBA SSE against the source as the encoder sees it: alpha 0 / 255 at its threshold,
                          RGB zeroed on transparent texels (the same bytes come out as from the raw source).  Alpha included:
                          the decoder's transparent texels are exactly the encoder's.
  ETC2 RGBA               colour error + EAC error = RGBA SSE;  EAC alpha: EAC error = alpha SSE
  BC1 (threshold 0.5, 0)  colour error + sum (255 - a)^2: PackRGB never emits the transparent index (its alpha test only
                          weights the end-point fit, S3TC.cpp:746-782, 967-1051), so every decoded texel is opaque
  BC2                     colour error + sum min_k (17 k - a)^2, k = 0..15 (PackExplicitAlpha keeps no error)
  BC3                     colour error + interpolated-alpha error;  BC4U / BC4S / BC5U / BC5S: the alpha error(s) of R (, G);
                          signed sources are int8 with -128 read as -127

Left out on purpose:
  * S3TC_Exhaustive (BC1-3 colour): the score TestCounts / TestSingleColor keep is not the SSE of the emitted block.
  * S3TC_Paranoid: adds a span term to every difference.
  * non-uniform channel weights and the FakeBT709 flags: weighted float arithmetic; the measure is unweighted by design.
  * R11: the encoder stores a base byte a spec decoder reads differently, so the two errors differ by
    construction.
  * BC7 / BC6H: already held to the reference's own decoders (tests/test_decode.py, test_decode_formats.py).
"""
import os

import numpy as np
import pytest

import content
import texture_decode_ref as R
from oracle import pyref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N = 1024
SIZES = (8, 264, 1024)  # one group in a partial wave; a second, ragged 256-block workgroup of the reduction; the mode coverage
FLOOR = 20              # every mode an anchor speaks for is seen in at least this many of the N blocks

# case -> (format name of decode / measure, the channels it stores)
CASES = {
    "etc2": ("etc2", (0, 1, 2)), "etc1": ("etc1", (0, 1, 2)), "etc2punchthrough": ("etc2punchthrough", (0, 1, 2, 3)),
    "etc2rgba": ("etc2rgba", (0, 1, 2, 3)), "eac": ("eac", (3,)),
    "bc1_t50": ("bc1", (0, 1, 2, 3)), "bc1_t0": ("bc1", (0, 1, 2, 3)), "bc2": ("bc2", (0, 1, 2, 3)), "bc3": ("bc3", (0, 1, 2, 3)),
    "bc4u": ("bc4u", (0,)), "bc4s": ("bc4s", (0,)), "bc5u": ("bc5u", (0, 1)), "bc5s": ("bc5s", (0, 1)),
}
ETC_MODE = {"etc2": 0, "etc2rgba": 1, "eac": 2, "etc1": 3, "etc2punchthrough": 4}
S3TC_FORMAT = {"bc2": 2, "bc3": 3, "bc4u": 4, "bc4s": 5, "bc5u": 6, "bc5s": 7}


def threshold_of(case):
    return 0.0 if case == "bc1_t0" else 0.5


def rcp_table():
    """one reciprocal table for the oracle and the device, whatever the host's RCPPS gives"""
    return np.load(os.path.join(GOLD, "s3tc_mixed.npz"))["rcp"]


# ---------------------------------------------------------------- source rules (the only statement of them here)

def punchthrough_threshold(threshold=0.5):
    """EncodeETC2PunchthroughAlpha: a texel is transparent when its alpha is below this"""
    return int(np.floor(np.float32(min(max(threshold, 0.0), 1.0)) * np.float32(255.0) + np.float32(1.0)))


def encoder_source(case, raw):
    """(N,16,4) the encoder is given for `case`, from raw RGBA8 content: int8 bit patterns for the signed formats; for
    punch-through the source as the encoder sees it -- alpha 0 / 255 at its threshold, RGB zeroed on transparent texels"""
    if case in ("bc4s", "bc5s"):
        return np.ascontiguousarray(raw).view(np.int8)
    if case == "etc2punchthrough":
        out = np.array(raw, np.uint8)
        transparent = out[:, :, 3] < punchthrough_threshold(threshold_of(case))
        out[:, :, 3] = np.where(transparent, 0, 255)
        out[transparent, :3] = 0
        return out
    return np.ascontiguousarray(raw)


def source_ints(source):
    """the source as the encoder reads it, int64: int8 sources read -128 as -127 (Util::BiasSignedInput)"""
    s = np.asarray(source)
    return np.maximum(s.astype(np.int64), -127) if s.dtype == np.int8 else s.astype(np.int64)


def block_sse(case, decoded, source, valid=None):
    """(N,) int64 squared error per block over the channels `case` stores; valid: (N,16) bool of the texels that count"""
    d = np.asarray(decoded).astype(np.int64) - source_ints(source)
    sq = (d * d)[:, :, list(CASES[case][1])].sum(axis=2)
    if valid is not None:
        sq = np.where(valid, sq, 0)
    return sq.sum(axis=1)


def to_int(err):
    """a float error of the oracle as int64, after checking that it is an integer a float holds exactly"""
    err = np.asarray(err)
    assert np.isfinite(err).all() and (err == np.floor(err)).all() and (err >= 0).all() and (err < 2.0 ** 24).all()
    return err.astype(np.int64)


# ---------------------------------------------------------------- content and the oracle's answer, computed once

def mixed_content():
    """content.mixed_ldr_blocks(424242, 128): its kinds cycle every 12 groups, so every prefix of SIZES past the first sees
    them all"""
    return content.mixed_ldr_blocks(424242, N // 8)


def punchthrough_content():
    """768 mixed blocks and the first 256 of content.punchthrough_blocks(5, 4), one cut-out group after every three mixed
    ones (whole groups of 8 move, so no block's encoding depends on the order)"""
    mixed = mixed_content()[:768].reshape(96, 8, 16, 4)
    cut = content.punchthrough_blocks(5, 4)[:256].reshape(32, 8, 16, 4)
    groups = []
    for i in range(32):
        groups += [mixed[3 * i], mixed[3 * i + 1], mixed[3 * i + 2], cut[i]]
    return np.ascontiguousarray(np.stack(groups).reshape(N, 16, 4))


def raw_content(case):
    return punchthrough_content() if case == "etc2punchthrough" else mixed_content()


def oracle_encode(orc, case, source):
    """(packed, expected per-block error int64, parts) of `source` under Flags::Uniform alone.  parts: the oracle's own
    numbers by name, for the CPU breakdowns."""
    opt = pyref.make_options(flags=pyref.FLAG_UNIFORM, threshold=threshold_of(case))
    rcp = rcp_table()
    src = np.ascontiguousarray(source).view(np.uint8)
    alpha = src[:, :, 3].astype(np.int64)
    if case in ETC_MODE:
        packed, cerr, aerr = orc.encode_etc2_err(src, opt, ETC_MODE[case], threads=8)
        parts = {}
        if cerr is not None:
            parts["colour"] = to_int(cerr)
        if aerr is not None:
            assert (aerr < 16 * 255 * 255 + 1).all()
            parts["alpha"] = aerr.astype(np.int64)
    elif case.startswith("bc1"):
        packed, err = orc.encode_bc1_err(src, opt, rcp, threads=8)
        # PackRGB emits opaque texels only (module docstring): the decoded alpha is 255 whatever the source's
        parts = {"colour": to_int(err), "alpha": ((255 - alpha) ** 2).sum(axis=1)}
    else:
        packed, cerr, aerr = orc.encode_s3tc_err(src, opt, S3TC_FORMAT[case], rcp, threads=8)
        parts = {}
        if cerr is not None:
            parts["colour"] = to_int(cerr)
        if case == "bc2":
            # PackExplicitAlpha keeps no error: from first principles, the nearest of the 16 levels 17 k
            levels = 17 * np.arange(16, dtype=np.int64)
            parts["alpha"] = ((levels[None, None, :] - alpha[:, :, None]) ** 2).min(axis=2).sum(axis=1)
        else:
            a = to_int(aerr)
            parts["alpha"] = a[:, 0]
            if a.shape[1] == 2:
                parts["alpha2"] = a[:, 1]
    return packed, sum(parts.values()), parts


_CACHE = {}


def anchor(orc, case):
    """(source, packed, expected error, parts) of the N blocks of `case`; computed once and shared, never modified"""
    if case not in _CACHE:
        source = encoder_source(case, raw_content(case))
        packed, err, parts = oracle_encode(orc, case, source)
        for a in (source, packed, err) + tuple(parts.values()):
            a.setflags(write=False)
        _CACHE[case] = (source, packed, err, parts)
    return _CACHE[case]


# ---------------------------------------------------------------- what the emitted bytes say (coverage only)

def etc_modes(colour):
    """mode of each (N,8) ETC colour block, read off the bytes.  ETC2 reading; `differential` is the diff bit, which
    punch-through blocks use as their opaque bit (they are always differential)."""
    b = colour.astype(np.int64)
    diff = (b[:, 3] >> 1) & 1 == 1

    def overflows(byte):
        delta = byte & 7
        v = (byte >> 3) + np.where(delta >= 4, delta - 8, delta)
        return (v < 0) | (v > 31)

    return diff, overflows(b[:, 0]), overflows(b[:, 1]), overflows(b[:, 2])


def etc_mode_counts(colour, punchthrough=False):
    diff, r, g, b = etc_modes(colour)
    differential = np.ones(len(colour), bool) if punchthrough else diff
    t = differential & r
    h = differential & ~r & g
    p = differential & ~r & ~g & b
    return {"individual": ~differential, "differential": differential & ~t & ~h & ~p, "T": t, "H": h, "planar": p}


def alpha_is_8_level(packed, off, signed):
    e = packed[:, off:off + 2].view(np.int8) if signed else packed[:, off:off + 2]
    return e[:, 0].astype(np.int64) > e[:, 1].astype(np.int64)


def assert_floor(mask, what):
    assert int(mask.sum()) >= FLOOR, (what, int(mask.sum()))


def check_coverage(case, source, packed):
    if case in ("etc2", "etc2rgba"):
        modes = etc_mode_counts(packed[:, -8:])
        for name in ("differential", "T", "H", "planar"):
            assert_floor(modes[name], (case, name))
    if case == "etc1":
        modes = etc_mode_counts(packed)
        # (ETC1 has no T / H / planar: its differential blocks never overflow)
        assert not (modes["T"] | modes["H"] | modes["planar"]).any()
        assert_floor(modes["individual"], (case, "individual"))
        assert_floor(modes["differential"], (case, "differential"))
    if case == "etc2punchthrough":
        opaque = etc_modes(packed)[0]
        transparent = source[:, :, 3] == 0
        assert_floor(opaque, (case, "opaque bit 1"))
        assert_floor(~opaque, (case, "opaque bit 0"))
        assert_floor(transparent.any(axis=1) & ~transparent.all(axis=1), (case, "some texels transparent"))
        assert_floor(transparent.all(axis=1), (case, "all texels transparent"))
        modes = etc_mode_counts(packed, punchthrough=True)
        for name in ("differential", "T", "H", "planar"):
            assert modes[name].any(), (case, name)
    if case.startswith("bc1"):
        c = packed.astype(np.int64)
        c0, c1 = c[:, 0] | (c[:, 1] << 8), c[:, 2] | (c[:, 3] << 8)
        assert_floor(c0 <= c1, (case, "three-colour"))
        assert_floor(c0 > c1, (case, "four-colour"))
    if case in S3TC_FORMAT and case != "bc2":
        signed = case.endswith("s")
        for off in ((0, 8) if case.startswith("bc5") else (0,)):
            full = alpha_is_8_level(packed, off, signed)
            assert_floor(full, (case, off, "8-level"))
            assert_floor(~full, (case, off, "6-level"))
    if case in ("bc4s", "bc5s"):
        for ch in CASES[case][1]:
            assert_floor((source[:, :, ch] == -128).any(axis=1), (case, ch, "-128 in the source"))


def prefix_modes_present(case, packed):
    """the 264-block prefix still holds a T, an H, a planar and -- punch-through -- a block with a transparent texel"""
    modes = etc_mode_counts(packed[:, -8:], punchthrough=(case == "etc2punchthrough"))
    return all(modes[name].any() for name in ("T", "H", "planar"))


# ---------------------------------------------------------------- CPU: the restatement against the encoder's number

@pytest.mark.parametrize("case", list(CASES))
def test_restatement_error_is_the_encoders(oracle_lib, case):
    source, packed, err, parts = anchor(oracle_lib, case)
    fmt, channels = CASES[case]
    assert len(packed) == N and err.shape == (N,)
    check_coverage(case, source, packed)
    decoded = R.decode(fmt, packed)
    got = block_sse(case, decoded, source)
    bad = np.nonzero(got != err)[0]
    assert bad.size == 0, (case, bad.size, bad[:8], got[bad[:8]], err[bad[:8]])
    # the parts, where the format has more than one: colour and alpha each equal their own number
    d = decoded.astype(np.int64) - source_ints(source)
    sq = (d * d).sum(axis=1)  # (N,4) per channel
    if "colour" in parts:
        assert (sq[:, :3].sum(axis=1) == parts["colour"] - (0 if case != "etc2punchthrough" else sq[:, 3])).all(), case
    if case in ("etc2rgba", "eac", "bc1_t50", "bc1_t0", "bc2", "bc3"):
        assert (sq[:, 3] == parts["alpha"]).all(), case
    if case in ("bc4u", "bc4s", "bc5u", "bc5s"):
        assert (sq[:, 0] == parts["alpha"]).all(), case
    if case in ("bc5u", "bc5s"):
        assert (sq[:, 1] == parts["alpha2"]).all(), case
    if case.startswith("bc1"):
        # what the alpha term rests on: no texel of a three-colour block carries the transparent index
        assert (decoded[:, :, 3] == 255).all()


def test_punchthrough_source_as_the_encoder_sees_it(oracle_lib):
    """the raw source and the one with alpha at 0 / 255 and transparent RGB zeroed encode to the same bytes with the same
    error, the transparent texels decode to (0,0,0,0) and the others to alpha 255, so the alpha part of the SSE is 0"""
    source, packed, err, parts = anchor(oracle_lib, "etc2punchthrough")
    raw = punchthrough_content()
    assert (raw != source).any()
    raw_packed, raw_err, _ = oracle_encode(oracle_lib, "etc2punchthrough", raw)
    assert (raw_packed == packed).all() and (raw_err == err).all()
    decoded = R.decode("etc2punchthrough", packed)
    transparent = source[:, :, 3] == 0
    assert (decoded[:, :, 3] == source[:, :, 3]).all()
    assert (decoded[transparent] == 0).all()
    assert transparent.any(axis=1).sum() >= 256 and transparent.all(axis=1).sum() >= 64


def test_prefixes_keep_the_modes(oracle_lib):
    """the shapes of the GPU tests: every prefix is whole groups, and the 264-block one still has T, H, planar and
    punch-through blocks to show"""
    assert all(n % 8 == 0 and n <= N for n in SIZES) and 256 < SIZES[1] < 512 and SIZES[1] % 256
    for case in ("etc2", "etc2rgba", "etc2punchthrough"):
        source, packed, _, _ = anchor(oracle_lib, case)
        assert prefix_modes_present(case, packed[:SIZES[1]]), case
    source, packed, _, _ = anchor(oracle_lib, "etc2punchthrough")
    transparent = (source[:SIZES[1], :, 3] == 0)
    assert (transparent.any(axis=1) & ~transparent.all(axis=1)).any() and transparent.all(axis=1).any()
    assert (~etc_modes(packed[:SIZES[1]])[0]).any()


def test_error_arrays_are_indexed_by_block(oracle_lib):
    """the errors of a multi-threaded run equal those of a single-threaded one, block for block, and the bytes those of
    the plain entry points"""
    src = mixed_content()[:264]
    opt = pyref.make_options(flags=pyref.FLAG_UNIFORM)
    rcp = rcp_table()
    for mode in range(5):
        one = oracle_lib.encode_etc2_err(src, opt, mode, threads=1)
        many = oracle_lib.encode_etc2_err(src, opt, mode, threads=5)
        assert (one[0] == oracle_lib.encode_etc2(src, opt, mode)).all()
        for a, b in zip(one, many):
            assert (a is None and b is None) or np.array_equal(a, b)
    for fmt in range(2, 8):
        one = oracle_lib.encode_s3tc_err(src, opt, fmt, rcp, threads=1)
        many = oracle_lib.encode_s3tc_err(src, opt, fmt, rcp, threads=5)
        assert (one[0] == oracle_lib.encode_s3tc(src, opt, fmt, rcp)).all()
        for a, b in zip(one, many):
            assert (a is None and b is None) or np.array_equal(a, b)
    one = oracle_lib.encode_bc1_err(src, opt, rcp, threads=1)
    many = oracle_lib.encode_bc1_err(src, opt, rcp, threads=5)
    assert (one[0] == oracle_lib.encode_bc1(src, opt, rcp)).all()
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])


# ---------------------------------------------------------------- GPU: decode and measure against the encoder's number

def gpu_encode(ctx, case, blocks, opt):
    """blocks: uint8 bit patterns, numpy or CUDA tensor"""
    if case in ("bc1_t50", "bc1_t0"):
        return ctx.encode_bc1(blocks, opt)
    simple = {"bc2": ctx.encode_bc2, "bc3": ctx.encode_bc3, "etc1": ctx.encode_etc1, "etc2": ctx.encode_etc2,
              "etc2rgba": ctx.encode_etc2_rgba, "eac": ctx.encode_etc2_alpha,
              "etc2punchthrough": ctx.encode_etc2_punchthrough_alpha}
    if case in simple:
        return simple[case](blocks, opt)
    if case in ("bc4u", "bc4s"):
        return ctx.encode_bc4(blocks, opt, signed=(case == "bc4s"))
    return ctx.encode_bc5(blocks, opt, signed=(case == "bc5s"))


def uniform_options(case):
    from convectionkernels_amd import api
    return api.Options(flags=api.Flags.Uniform, threshold=threshold_of(case))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_error_is_the_encoders(gpu_ctx, oracle_lib, case, n):
    import torch
    source, packed, err, _ = anchor(oracle_lib, case)
    source, packed, err = source[:n], packed[:n], err[:n]
    fmt, channels = CASES[case]
    mask = sum(1 << c for c in channels)
    gpu_ctx.set_rcp_table(rcp_table())
    opt = uniform_options(case)
    host_source = np.array(source)  # (the shared arrays are read-only; torch wants a writable one)
    host_packed = np.array(packed)
    for device in (False, True):
        if device:
            src = torch.from_numpy(host_source).cuda()
            pk = gpu_encode(gpu_ctx, case, src.view(torch.uint8), opt)
            got_packed = pk.cpu().numpy()
        else:
            src = host_source
            pk = got_packed = gpu_encode(gpu_ctx, case, host_source.view(np.uint8), opt)
        bad = np.nonzero((got_packed != host_packed).any(axis=1))[0]
        assert bad.size == 0, (case, n, device, "bytes", bad[:8])
        rep = gpu_ctx.measure_error(fmt, src, pk, per_block=True)
        pb = rep.per_block.cpu().numpy() if device else rep.per_block
        assert rep.texels == 16 * n and rep.channel_mask == mask
        bad = np.nonzero(pb.astype(np.int64) != err)[0]
        assert bad.size == 0, (case, n, device, "per_block", bad[:8], pb[bad[:8]], err[bad[:8]])
        assert all(int(rep.totals.sse[c]) == 0 for c in range(4) if c not in channels)
        assert sum(int(rep.totals.sse[c]) for c in channels) == int(err.sum()), (case, n, device, "totals")
        dec = gpu_ctx.decode(fmt, pk)
        dec = dec.cpu().numpy() if device else dec
        assert dec.dtype == host_source.dtype
        got = block_sse(case, dec, host_source)
        bad = np.nonzero(got != err)[0]
        assert bad.size == 0, (case, n, device, "decode", bad[:8], got[bad[:8]], err[bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["etc2", "bc3"])
def test_gpu_measure_image_is_the_encoders(gpu_ctx, oracle_lib, case):
    """a 37 x 23 image: its blocks are the oracle's encoding of the clamped tiles, and the measure is the oracle's error
    less that of the texels outside the image, which the clamped tiles hold and the image does not"""
    import torch
    w, h = 37, 23
    rng = np.random.Generator(np.random.PCG64(3723))
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(x * 7) & 255, (y * 11) & 255, (3 * x + 5 * y) & 255, (255 - 6 * x - 2 * y) & 255], -1).astype(np.uint8)
    img ^= rng.integers(0, 32, img.shape, dtype=np.uint8)
    fmt, channels = CASES[case]
    tiles = content.tile_clamped(img)
    packed, err, _ = oracle_encode(oracle_lib, case, tiles)
    bw, bh = (w + 3) // 4, (h + 3) // 4
    per_row = len(tiles) // bh
    keep = (np.arange(len(tiles)) % per_row) < bw
    tiles, packed, err = tiles[keep], np.ascontiguousarray(packed[keep]), err[keep]
    assert len(packed) == bw * bh
    bx, by = np.arange(bw * bh) % bw, np.arange(bw * bh) // bw
    px, py = np.arange(16) % 4, np.arange(16) // 4
    valid = ((4 * bx[:, None] + px[None, :]) < w) & ((4 * by[:, None] + py[None, :]) < h)
    assert int(valid.sum()) == w * h and (~valid).any(axis=1).sum() == bw + bh - 1

    gpu_ctx.set_rcp_table(rcp_table())
    dev = torch.from_numpy(img).cuda()
    got = gpu_ctx.encode_image(fmt, dev, uniform_options(case))
    assert (got.cpu().numpy() == packed).all(), case
    padded = np.concatenate([packed, np.zeros(((-len(packed)) % 8, packed.shape[1]), np.uint8)])
    decoded = gpu_ctx.decode(fmt, padded)[:len(packed)]
    outside = block_sse(case, decoded, tiles, ~valid)
    assert (block_sse(case, decoded, tiles) == err).all(), case
    assert outside.sum() > 0
    expect = err - outside
    rep = gpu_ctx.measure_image(fmt, dev, got, per_block=True)
    assert rep.texels == w * h and rep.channel_mask == sum(1 << c for c in channels)
    pb = rep.per_block.cpu().numpy().astype(np.int64)
    bad = np.nonzero(pb != expect)[0]
    assert bad.size == 0, (case, bad[:8], pb[bad[:8]], expect[bad[:8]])
    assert sum(int(rep.totals.sse[c]) for c in channels) == int(expect.sum()), case
