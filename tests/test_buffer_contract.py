"""The buffer contract of the C ABI (include/cvtt_mi355x.h, "Buffers"): every device entry point writes exactly its output --
every byte of it, and none outside -- reads its input only, and works on any block-aligned slice of a larger allocation.

The other GPU tests read back the tensor a call returned; a kernel that skips a lane, a group, a half-block or a ragged tail
passes them when the caching allocator hands the loop the previous, correct answer, and nothing looks past out[n].  Here
every call goes through the raw C ABI (gpu_ctx._lib, data_ptr() values) into poisoned, guarded allocations
(tests/guarded.py), with input and output 0, 1 and 3 blocks into their allocations, at the smallest sizes at which each
launch shape has a ragged edge, and with two poison values.  Expected bytes never come from another GPU call: the C oracle
(once per format on 1032 blocks; the sizes are whole 8-block groups, so every prefix is valid), the numpy decoders and
measure of texture_decode_ref.py, tests/golden/decode.npz for BC7 / BC6H, and content.tile_clamped / compact_rows.

CPU: the helper's self-tests and "no expected granule equals a poison granule", so an unwritten block can never pass."""
import ctypes
import os

import numpy as np
import pytest

import content
import guarded
import texture_decode_ref as R
from convectionkernels_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

POISONS = (0xA5, 0x5A)
# 8: less than a wave in every kernel; 24; 72: no multiple of 16 or 64; 264: a second, ragged 256-block workgroup;
# 1032: 129 groups, no multiple of the eight XCDs the ETC2 groups are dealt to
SIZES = (8, 24, 72, 264, 1032)
FULL = SIZES[-1]
# either side of the switch between the two EAC launch forms (sixteen lanes / one lane per block, etc2_kernel.hip)
EAC_SIZES = (65536, 65544)
BLOCK_OFFSETS = (0, 1, 3)  # input and output start this many blocks of their own size into their allocation
COMBOS = [(i, o) for i in BLOCK_OFFSETS for o in BLOCK_OFFSETS]
E_INVALID = -1


def _addr(s):
    return ctypes.addressof(s)


def _opt_bytes(opt):
    return np.frombuffer(opt.tobytes(), np.uint8).copy()


def _rcp():
    return np.load(os.path.join(GOLD, "s3tc_mixed.npz"))["rcp"]


# ---------------------------------------------------------------- content and expected bytes (computed once, never changed)

_CONTENT = {}


def source_blocks(kind):
    """FULL blocks of the encoder input of `kind`"""
    if kind not in _CONTENT:
        if kind == "ldr":
            b = content.mixed_ldr_blocks(4242, FULL // 8)
        elif kind == "hdru":
            b = content.mixed_hdr_blocks(4243, FULL // 8, signed=False)
        elif kind == "hdrs":
            b = content.mixed_hdr_blocks(4244, FULL // 8, signed=True)
        elif kind == "r11":
            b = content.mixed_r11_blocks(4245, FULL // 8)
        else:  # "pt": every kind of punch-through alpha, 129 of its 140 groups spread evenly
            g = content.punchthrough_blocks(7, 10).reshape(-1, 8, 16, 4)
            b = g[np.linspace(0, len(g) - 1, FULL // 8).astype(int)].reshape(FULL, 16, 4)
        b = np.ascontiguousarray(b)
        b.setflags(write=False)
        _CONTENT[kind] = b
    return _CONTENT[kind]


def _simple(name):
    return lambda lib, h, o, i, n, opt: getattr(lib, name)(h, o, i, n, _addr(opt), None)


_PLAN = api.BC7EncodingPlan()
_ALLOC_OPT = api.Options(redWeight=1.0, greenWeight=0.5, blueWeight=0.25)  # what AllocETC2Data was given (with_data)

# name -> (content kind, input bytes per block, output bytes per block, device call, oracle call,
#          non-default Options (kwargs) that switch the kernel variant, run at 264 blocks, or None)
ENCODERS = {
    "bc7": ("ldr", 64, 16,
            lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc7_device(h, o, i, n, _addr(opt), _addr(_PLAN), None),
            lambda orc, b, ob, rcp: orc.encode_bc7(b, ob, _opt_bytes(_PLAN), rcp, threads=8),
            # Flags::Better (no fast indexing), punch-through, 7 refine rounds: the trial table in HBM
            dict(flags=api.Flags.Better | api.Flags.BC7_RespectPunchThrough, refineRoundsBC7=7)),
    "bc1": ("ldr", 64, 8, _simple("cvttmi_encode_bc1_device"), lambda orc, b, ob, rcp: orc.encode_bc1(b, ob, rcp, threads=8),
            dict(flags=api.Flags.Better)),
    "bc2": ("ldr", 64, 16, _simple("cvttmi_encode_bc2_device"), lambda orc, b, ob, rcp: orc.encode_s3tc(b, ob, 2, rcp, threads=8),
            dict(flags=api.Flags.Better)),
    "bc3": ("ldr", 64, 16, _simple("cvttmi_encode_bc3_device"), lambda orc, b, ob, rcp: orc.encode_s3tc(b, ob, 3, rcp, threads=8),
            dict(flags=api.Flags.Better)),
    "bc4u": ("ldr", 64, 8, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc4_device(h, o, i, n, _addr(opt), 0, None),
             lambda orc, b, ob, rcp: orc.encode_s3tc(b, ob, 4, rcp, threads=8), None),
    "bc4s": ("ldr", 64, 8, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc4_device(h, o, i, n, _addr(opt), 1, None),
             lambda orc, b, ob, rcp: orc.encode_s3tc(b, ob, 5, rcp, threads=8), None),
    "bc5u": ("ldr", 64, 16, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc5_device(h, o, i, n, _addr(opt), 0, None),
             lambda orc, b, ob, rcp: orc.encode_s3tc(b, ob, 6, rcp, threads=8), None),
    "bc5s": ("ldr", 64, 16, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc5_device(h, o, i, n, _addr(opt), 1, None),
             lambda orc, b, ob, rcp: orc.encode_s3tc(b, ob, 7, rcp, threads=8), None),
    "bc6hu": ("hdru", 128, 16, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc6h_device(h, o, i, n, _addr(opt), 0, None),
              lambda orc, b, ob, rcp: orc.encode_bc6h(b, ob, False, rcp, threads=8),
              dict(flags=api.Flags.Default | api.Flags.BC6H_FastIndexing, seedPoints=3)),
    "bc6hs": ("hdrs", 128, 16, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc6h_device(h, o, i, n, _addr(opt), 1, None),
              lambda orc, b, ob, rcp: orc.encode_bc6h(b, ob, True, rcp, threads=8), None),
    "etc1": ("ldr", 64, 8, _simple("cvttmi_encode_etc1_device"), lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 3, threads=8), None),
    "etc2": ("ldr", 64, 8, _simple("cvttmi_encode_etc2_device"), lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 0, threads=8), None),
    "etc2rgba": ("ldr", 64, 16, _simple("cvttmi_encode_etc2_rgba_device"), lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 1, threads=8), None),
    "etc2alpha": ("ldr", 64, 8, _simple("cvttmi_encode_etc2_alpha_device"), lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 2, threads=8), None),
    "etc2punchthrough": ("pt", 64, 8, _simple("cvttmi_encode_etc2_punchthrough_alpha_device"),
                         lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 4, threads=8), None),
    "r11u": ("r11", 32, 8, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_alpha11_device(h, o, i, n, 0, _addr(opt), None),
             lambda orc, b, ob, rcp: orc.encode_eac11(b, False), None),
    "r11s": ("r11", 32, 8, lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_alpha11_device(h, o, i, n, 1, _addr(opt), None),
             lambda orc, b, ob, rcp: orc.encode_eac11(b, True), None),
    # the three kinds that take the reference's ETC2CompressionData, allocated with other weights than the encode's
    "with_data_rgb": ("ldr", 64, 8,
                      lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_with_data_device(h, o, i, n, _addr(opt), _addr(_ALLOC_OPT), 0, None),
                      lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 0, threads=8, alloc_options=_opt_bytes(_ALLOC_OPT)), None),
    "with_data_rgba": ("ldr", 64, 16,
                       lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_with_data_device(h, o, i, n, _addr(opt), _addr(_ALLOC_OPT), 1, None),
                       lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 1, threads=8, alloc_options=_opt_bytes(_ALLOC_OPT)), None),
    "with_data_punchthrough": ("pt", 64, 8,
                               lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_with_data_device(h, o, i, n, _addr(opt), _addr(_ALLOC_OPT), 4, None),
                               lambda orc, b, ob, rcp: orc.encode_etc2(b, ob, 4, threads=8, alloc_options=_opt_bytes(_ALLOC_OPT)), None),
}
EAC_ENTRIES = ("etc2alpha", "r11u", "r11s")
VARIANT_BLOCKS = 264

_EXPECTED = {}


def expected_encoding(orc, name, variant=False):
    """the oracle's packed blocks: FULL blocks with default Options, or VARIANT_BLOCKS with the entry's non-default set"""
    key = (name, variant)
    if key not in _EXPECTED:
        kind, _, out_bpb, _, oracle, kw = ENCODERS[name]
        opt = api.Options(**kw) if variant else api.Options()
        n = VARIANT_BLOCKS if variant else FULL
        out = np.ascontiguousarray(oracle(orc, source_blocks(kind)[:n], _opt_bytes(opt), _rcp())).reshape(n, out_bpb)
        out.setflags(write=False)
        _EXPECTED[key] = out
    return _EXPECTED[key]


DECODE_FORMATS = ["bc7", "bc1", "bc6hu", "bc6hs", "etc2", "etc2rgba", "bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s", "etc1",
                  "etc2punchthrough", "eac", "r11u", "r11s"]
assert [api.TEXTURE_FORMATS[f][0] for f in DECODE_FORMATS] == list(range(17))
_DECODE = {}


def decode_case(fmt):
    """(packed (FULL, bytes) uint8, decoded blocks) of `fmt`: BC7 / BC6H from the reference's decoder (tests/golden/decode.npz),
    every other format seeded random blocks through the numpy decoders"""
    if fmt not in _DECODE:
        if fmt in ("bc7", "bc6hu", "bc6hs"):
            g = np.load(os.path.join(GOLD, "decode.npz"))
            key = {"bc7": "bc7", "bc6hu": "bc6u", "bc6hs": "bc6s"}[fmt]
            packed, dec = g[key + "_in"][:FULL], g[key + "_out"][:FULL]
        else:
            fid, bpb = api.TEXTURE_FORMATS[fmt][:2]
            packed = np.random.Generator(np.random.PCG64(9100 + fid)).integers(0, 256, (FULL, bpb), dtype=np.uint8)
            dec = R.decode(fmt, packed)
        packed, dec = np.ascontiguousarray(packed), np.ascontiguousarray(dec)
        assert len(packed) == FULL and dec.nbytes == FULL * api.TEXTURE_FORMATS[fmt][2]
        packed.setflags(write=False)
        dec.setflags(write=False)
        _DECODE[fmt] = (packed, dec)
    return _DECODE[fmt]


_MEASURE_SRC = {}


def measure_source(fmt):
    """FULL source blocks in the layout the format's encoder reads (finite values: no NaN in any expected value)"""
    if fmt not in _MEASURE_SRC:
        rng = np.random.Generator(np.random.PCG64(9500 + api.TEXTURE_FORMATS[fmt][0]))
        if fmt in ("bc6hu", "bc6hs"):
            s = rng.uniform(-2.0 if fmt == "bc6hs" else 0.0, 4.0, (FULL, 16, 4)).astype(np.float16).view(np.int16)
        elif fmt in ("r11u", "r11s"):
            s = rng.integers(-1200, 2200, (FULL, 16), dtype=np.int16)  # outside the encoder's range too: it clamps
        else:
            s = rng.integers(0, 256, (FULL, 16, 4), dtype=np.uint8)
        s.setflags(write=False)
        _MEASURE_SRC[fmt] = s
    return _MEASURE_SRC[fmt]


def totals_bytes(fmt, exp):
    t = api.ErrorTotals()
    for c in range(4):
        t.sse[c] = int(exp["sse"][c])
        t.sseHdr[c] = float(exp["sse_hdr"][c])
    t.texels = int(exp["texels"])
    t.channelMask = R.FORMATS[fmt][2]
    t.format = R.FORMATS[fmt][0]
    return bytes(t)


_MEASURE = {}


def measure_case(fmt, n):
    """(80 bytes of totals, per-block values) of the first n blocks of the decode case against measure_source"""
    if (fmt, n) not in _MEASURE:
        exp, per_block = R.measure(fmt, decode_case(fmt)[1][:n], measure_source(fmt)[:n])
        assert np.isfinite(np.asarray(exp["sse_hdr"], np.float64)).all() and np.isfinite(per_block.astype(np.float64)).all()
        _MEASURE[(fmt, n)] = (totals_bytes(fmt, exp), np.ascontiguousarray(per_block))
    return _MEASURE[(fmt, n)]


def make_image(w, h, hdr, seed=0):
    """(h, w, 4) uint8, or int16 half bit patterns (finite, alpha 1.0): noise, every texel different from the poisons"""
    rng = np.random.Generator(np.random.PCG64(100 * w + h + seed + (7 if hdr else 0)))
    if hdr:
        img = rng.uniform(0.0, 8.0, (h, w, 4)).astype(np.float16).view(np.int16)
        img[..., 3] = 0x3C00
        return img
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


TILE_SIZES = ((37, 10), (1, 1), (33, 5))
ROUTE_SIZE = (75, 22)


def route_case(orc, fmt):
    """the encode_image route of `fmt` at ROUTE_SIZE: (image, tiles, packed tiles, compacted rows), the packed ones by the
    oracle on the clamped tiles"""
    key = ("route", fmt)
    if key not in _EXPECTED:
        w, h = ROUTE_SIZE
        img = make_image(w, h, fmt == "bc6hu", seed=3)
        tiles = content.tile_clamped(img)
        ob = _opt_bytes(api.Options())
        packed = orc.encode_bc6h(tiles, ob, False, _rcp(), threads=8) if fmt == "bc6hu" else orc.encode_etc2(tiles, ob, 0, threads=8)
        _EXPECTED[key] = (img, tiles, np.ascontiguousarray(packed), content.compact_rows(packed, w, h))
    return _EXPECTED[key]


# ---------------------------------------------------------------- CPU: the helper, and the poison can never pass

def test_guard_reports_a_byte_before_and_after_the_payload():
    exp = np.arange(64, dtype=np.uint8)
    # the last byte of the front guard (the gap is 8 bytes), a byte of the gap, the first byte of the back guard
    for where, index in (("front guard", -9), ("offset gap", -1), ("back guard", 64)):
        view, check = guarded.host_buffer(64, offset=8, poison=0xA5)
        view[:] = exp
        check(exp)
        raw = check._snapshot()  # (numpy: the live allocation)
        raw[check.front + check.offset + index] = 0x00
        with pytest.raises(AssertionError) as e:
            check(exp)
        msg = str(e.value)
        assert where in msg and "offsets %d .. %d" % (index, index) in msg and "1 byte(s)" in msg, msg


def test_guard_reports_an_unwritten_block():
    for poison in POISONS:
        view, check = guarded.host_buffer(256, offset=3, poison=poison)
        exp = (np.arange(256) * 7 % 251).astype(np.uint8)
        view[:] = exp
        view[40:48] = poison  # a kernel that skipped one 8-byte block
        with pytest.raises(AssertionError) as e:
            check(exp)
        assert "offsets 40 .. 47" in str(e.value) and "8 payload byte(s)" in str(e.value) and "8 of them still hold" in str(e.value)
        with pytest.raises(AssertionError) as e:
            check.no_poison_blocks(8)
        assert "offsets 40 .. 47" in str(e.value)
        view[40:48] = exp[40:48]
        check(exp)
        check.no_poison_blocks(8)
    view, check = guarded.host_buffer(32, poison=0x5A)
    check.untouched()
    view[31] = 1
    with pytest.raises(AssertionError):
        check.untouched()


def _granules(a, g):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8).reshape(-1, g)


def test_no_expected_block_equals_a_poison_block(oracle_lib):
    """Every expected output of every case below, cut into the smallest unit any kernel stores at once (8 bytes: an 8-byte
    block, a BC2 / BC3 / BC5 half, two decoded texels; 4 bytes for the measure's per-block values), differs from that unit
    of either poison -- so a block a kernel did not write can never compare equal."""
    outputs = []
    for name, (_, _, _, _, _, kw) in ENCODERS.items():
        outputs.append((name, expected_encoding(oracle_lib, name), 8))
        if kw:
            outputs.append((name + " variant", expected_encoding(oracle_lib, name, True), 8))
    for fmt in DECODE_FORMATS:
        outputs.append(("decode " + fmt, decode_case(fmt)[1], 8))
        for n in SIZES:
            tot, pb = measure_case(fmt, n)
            outputs.append(("per-block " + fmt, pb, 4))
            outputs.append(("totals " + fmt, np.frombuffer(tot, np.uint8), 80))
    for w, h in TILE_SIZES:
        for hdr in (False, True):
            outputs.append(("tiles", content.tile_clamped(make_image(w, h, hdr)), 8))
    for fmt in ("etc2", "bc6hu"):
        _, tiles, packed, rows = route_case(oracle_lib, fmt)
        outputs += [("route tiles", tiles, 8), ("route packed", packed, 8), ("route rows", rows, 8)]
    for name, arr, g in outputs:
        cut = _granules(arr, g)
        for poison in POISONS:
            assert not (cut == poison).all(axis=1).any(), (name, hex(poison))


# ---------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    """the shared context with the reciprocal table the expected bytes were computed with (restored afterwards)"""
    before = gpu_ctx.get_rcp_table()
    gpu_ctx.set_rcp_table(_rcp())
    yield gpu_ctx
    gpu_ctx.set_rcp_table(before)


def _bytes(a):
    return np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", list(ENCODERS))
def test_device_encoders_write_exactly_their_output(ctx, oracle_lib, name, poison):
    lib, h = ctx._lib, ctx._h
    kind, in_bpb, out_bpb, call, _, kw = ENCODERS[name]
    blocks, exp = source_blocks(kind), expected_encoding(oracle_lib, name)
    opt = api.Options()
    for n in SIZES:
        for in_off, out_off in COMBOS:
            what = "%s, %d blocks, input +%d, output +%d blocks" % (name, n, in_off, out_off)
            src, unchanged = guarded.device_input(blocks[:n], in_off * in_bpb, what=what + ": input")
            out, check = guarded.device_buffer(n * out_bpb, out_off * out_bpb, poison, what=what)
            assert call(lib, h, out.data_ptr(), src.data_ptr(), n, opt) == 0, (what, lib.cvttmi_last_error(h))
            check(exp[:n])
            unchanged()
    if kw:
        vopt, vexp = api.Options(**kw), expected_encoding(oracle_lib, name, True)
        n = VARIANT_BLOCKS
        for in_off, out_off in ((0, 0), (1, 3), (3, 1)):
            what = "%s with %s, %d blocks, input +%d, output +%d blocks" % (name, kw, n, in_off, out_off)
            src, unchanged = guarded.device_input(blocks[:n], in_off * in_bpb, what=what + ": input")
            out, check = guarded.device_buffer(n * out_bpb, out_off * out_bpb, poison, what=what)
            assert call(lib, h, out.data_ptr(), src.data_ptr(), n, vopt) == 0, (what, lib.cvttmi_last_error(h))
            check(vexp)
            unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("n", EAC_SIZES)
@pytest.mark.parametrize("name", EAC_ENTRIES)
def test_eac_launch_forms(ctx, oracle_lib, name, n, poison):
    """65 536 blocks: the last launch of sixteen lanes per block; 65 544: the first of one lane per block, with a ragged
    last wave.  The content is the FULL blocks repeated, so the oracle's bytes of the first and the last FULL blocks are
    rotations of its one run (groups are independent); the blocks between are checked for poison left behind."""
    lib, h = ctx._lib, ctx._h
    kind, in_bpb, out_bpb, call, _, _ = ENCODERS[name]
    base, exp = source_blocks(kind), expected_encoding(oracle_lib, name)
    idx = np.arange(n) % FULL
    blocks = base[idx]
    opt = api.Options()
    for in_off, out_off in COMBOS:
        what = "%s, %d blocks, input +%d, output +%d blocks" % (name, n, in_off, out_off)
        src, unchanged = guarded.device_input(blocks, in_off * in_bpb, what=what + ": input")
        out, check = guarded.device_buffer(n * out_bpb, out_off * out_bpb, poison, what=what)
        assert call(lib, h, out.data_ptr(), src.data_ptr(), n, opt) == 0, (what, lib.cvttmi_last_error(h))
        got = check.payload().reshape(n, out_bpb)  # (guards are checked below)
        assert (got[:FULL] == exp[idx[:FULL]]).all(), what + ": first %d blocks" % FULL
        assert (got[-FULL:] == exp[idx[-FULL:]]).all(), what + ": last %d blocks" % FULL
        check.no_poison_blocks(out_bpb)
        check(got)  # guards and gap intact
        unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("fmt", DECODE_FORMATS)
def test_device_decoders_write_exactly_their_output(ctx, fmt, poison):
    lib, h = ctx._lib, ctx._h
    fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
    packed, dec = decode_case(fmt)
    dec = _bytes(dec).reshape(FULL, tex)
    for n in SIZES:
        for in_off, out_off in COMBOS:
            what = "decode %s, %d blocks, input +%d, output +%d blocks" % (fmt, n, in_off, out_off)
            src, unchanged = guarded.device_input(packed[:n], in_off * bpb, what=what + ": input")
            out, check = guarded.device_buffer(n * tex, out_off * tex, poison, what=what)
            assert lib.cvttmi_decode_device(h, fid, out.data_ptr(), src.data_ptr(), n, None) == 0, (what, lib.cvttmi_last_error(h))
            check(dec[:n])
            unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("fmt", DECODE_FORMATS)
def test_measure_overwrites_its_totals_and_values(ctx, fmt, poison):
    """cvttmi_measure_error_device: the per-block values and the 80 bytes of totals, each guarded, the totals poisoned
    beforehand -- the header says a call overwrites them, so the poison must be gone and nothing of it added in; also with
    the per-block pointer NULL."""
    lib, h = ctx._lib, ctx._h
    fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
    packed, source = decode_case(fmt)[0], measure_source(fmt)
    for n in SIZES:
        tot_exp, pb_exp = measure_case(fmt, n)
        for k, (bc_off, src_off) in enumerate(COMBOS):
            small = BLOCK_OFFSETS[k % 3]  # per-block values start 0, 1, 3 values in; the totals 0, 8, 24 bytes
            what = "measure %s, %d blocks, packed +%d, source +%d blocks, values +%d, totals +%d bytes" % (fmt, n, bc_off, src_off, small, 8 * small)
            bc, bc_same = guarded.device_input(packed[:n], bc_off * bpb, what=what + ": packed")
            src, src_same = guarded.device_input(source[:n], src_off * tex, what=what + ": source")
            tot, tot_check = guarded.device_buffer(80, 8 * small, poison, what=what + ": totals")
            with_values = k != 4
            pb, pb_check = guarded.device_buffer(n * 4, 4 * small, poison, what=what + ": per-block values")
            rc = lib.cvttmi_measure_error_device(h, fid, bc.data_ptr(), src.data_ptr(), n, pb.data_ptr() if with_values else None,
                                                 tot.data_ptr(), None)
            assert rc == 0, (what, lib.cvttmi_last_error(h))
            tot_check(tot_exp)
            if with_values:
                pb_check(pb_exp)
            else:
                pb_check.untouched()
            bc_same()
            src_same()


def _pitched(img, pitch_texels, filler):
    """img (h, w, 4) inside rows of pitch_texels texels; the padding holds `filler`"""
    h, w = img.shape[:2]
    rows = np.full((h, pitch_texels, 4), filler, img.dtype)
    rows[:, :w] = img
    # (the last row of an image needs only `w` texels: hand over exactly that, so reading the padding of the last row would
    # still stay inside the allocation's guard)
    return rows.reshape(-1)[: ((h - 1) * pitch_texels + w) * 4]


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
def test_measure_image_with_a_wide_pitch(ctx, oracle_lib, poison):
    """cvttmi_measure_image_error_device on 37 x 23 (clipped last block column and row), rows 43 texels apart"""
    lib, h = ctx._lib, ctx._h
    w, hh, pitch = 37, 23, 43
    nb = ((w + 3) // 4) * ((hh + 3) // 4)
    for fmt in ("bc1", "etc2rgba", "bc6hu"):
        fid, bpb, _, _ = api.TEXTURE_FORMATS[fmt]
        hdr = fmt == "bc6hu"
        texel = 8 if hdr else 4
        img = make_image(w, hh, hdr, seed=1)
        packed, dec = decode_case(fmt)[0][:nb], decode_case(fmt)[1][:nb]
        blocks, valid = R.image_to_blocks(img, fmt)
        exp, pb_exp = R.measure(fmt, dec, blocks, valid)
        assert exp["texels"] == w * hh
        flat = _pitched(img, pitch, 0x7B if not hdr else 0x3555)
        for k in BLOCK_OFFSETS:
            what = "measure_image %s, image +%d texels, packed +%d blocks" % (fmt, k, k)
            image, image_same = guarded.device_input(flat, k * texel, what=what + ": image")
            bc, bc_same = guarded.device_input(packed, k * bpb, what=what + ": packed")
            tot, tot_check = guarded.device_buffer(80, 8 * k, poison, what=what + ": totals")
            pb, pb_check = guarded.device_buffer(nb * 4, 4 * k, poison, what=what + ": per-block values")
            rc = lib.cvttmi_measure_image_error_device(h, fid, bc.data_ptr(), image.data_ptr(), w, hh, pitch * texel, 1 if hdr else 0,
                                                       pb.data_ptr(), tot.data_ptr(), None)
            assert rc == 0, (what, lib.cvttmi_last_error(h))
            tot_check(totals_bytes(fmt, exp))
            pb_check(pb_exp)
            image_same()
            bc_same()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("size", TILE_SIZES)
def test_tile_and_compact(ctx, size, poison):
    """cvttmi_tile_image_device (clamped padding blocks, a pitch wider than the image) and cvttmi_compact_rows_device"""
    lib, h = ctx._lib, ctx._h
    w, hh = size
    pitch = w + 5
    n_tiles = ((w + 3) // 4 + 7) // 8 * 8 * ((hh + 3) // 4)
    assert n_tiles == lib.cvttmi_tiled_block_count(w, hh)
    for hdr in (False, True):
        texel = 8 if hdr else 4
        img = make_image(w, hh, hdr)
        exp = content.tile_clamped(img)
        flat = _pitched(img, pitch, 0x7B if not hdr else 0x3555)
        for in_off, out_off in COMBOS:
            what = "tile %dx%d %s, image +%d texels, blocks +%d blocks" % (w, hh, "RGBA16F" if hdr else "RGBA8", in_off, out_off)
            image, image_same = guarded.device_input(flat, in_off * texel, what=what + ": image")
            out, check = guarded.device_buffer(n_tiles * 16 * texel, out_off * 16 * texel, poison, what=what)
            rc = lib.cvttmi_tile_image_device(h, out.data_ptr(), image.data_ptr(), w, hh, pitch * texel, 1 if hdr else 0, None)
            assert rc == 0, (what, lib.cvttmi_last_error(h))
            check(exp)
            image_same()
    for bpb in (8, 16):
        packed = np.random.Generator(np.random.PCG64(w * 31 + hh + bpb)).integers(1, 256, (n_tiles, bpb), dtype=np.uint8) & 0xDF
        packed |= 1  # (no byte equals either poison)
        exp = content.compact_rows(packed, w, hh)
        for in_off, out_off in COMBOS:
            what = "compact %dx%d, %d-byte blocks, input +%d, output +%d blocks" % (w, hh, bpb, in_off, out_off)
            src, same = guarded.device_input(packed, in_off * bpb, what=what + ": input")
            out, check = guarded.device_buffer(exp.nbytes, out_off * bpb, poison, what=what)
            assert lib.cvttmi_compact_rows_device(h, out.data_ptr(), src.data_ptr(), w, hh, bpb, None) == 0, (what, lib.cvttmi_last_error(h))
            check(exp)
            same()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("fmt", ["bc6hu", "etc2"])
def test_encode_image_route(ctx, oracle_lib, fmt, poison):
    """tile -> encode -> compact at 75 x 22 (19 real blocks in rows of 24, a clipped last block row) for the two formats whose
    groups are coupled and that tests/test_tiling.py does not cover: BC6HU from an RGBA16F image and ETC2 RGB, each step into
    a guarded buffer, against the oracle on the clamped tiles"""
    lib, h = ctx._lib, ctx._h
    w, hh = ROUTE_SIZE
    img, tiles, packed, rows = route_case(oracle_lib, fmt)
    hdr = fmt == "bc6hu"
    texel = 8 if hdr else 4
    n = len(tiles)
    assert n == 24 * 6 and len(rows) == 19 * 6
    opt = api.Options()
    for k in BLOCK_OFFSETS:
        what = "%s image route, every buffer +%d" % (fmt, k)
        image, image_same = guarded.device_input(img, k * texel, what=what + ": image")
        d_tiles, tiles_check = guarded.device_buffer(tiles.nbytes, k * 16 * texel, poison, what=what + ": tiles")
        d_packed, packed_check = guarded.device_buffer(packed.nbytes, k * packed.shape[1], poison, what=what + ": packed")
        d_rows, rows_check = guarded.device_buffer(rows.nbytes, k * packed.shape[1], poison, what=what + ": rows")
        assert lib.cvttmi_tile_image_device(h, d_tiles.data_ptr(), image.data_ptr(), w, hh, w * texel, 1 if hdr else 0, None) == 0
        if hdr:
            assert lib.cvttmi_encode_bc6h_device(h, d_packed.data_ptr(), d_tiles.data_ptr(), n, _addr(opt), 0, None) == 0
        else:
            assert lib.cvttmi_encode_etc2_device(h, d_packed.data_ptr(), d_tiles.data_ptr(), n, _addr(opt), None) == 0
        assert lib.cvttmi_compact_rows_device(h, d_rows.data_ptr(), d_packed.data_ptr(), w, hh, packed.shape[1], None) == 0
        tiles_check(tiles)
        packed_check(packed)
        rows_check(rows)
        image_same()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("punchthrough_between", [True, False])
def test_stale_hand_over_records_stay_inside_a_smaller_encode(oracle_lib, monkeypatch, punchthrough_between, poison):
    """The second BC7 launch stores through rec.blockIndex, read back from the hand-over list in HBM.  After an encode that
    handed blocks over (and, in one form, a punch-through encode, which gets no slots and clears no counter), an encode of
    264 blocks on the same context must not act on the larger encode's records: they point past its output.  The back
    guard is as large as the first encode's whole output, so a stale record would land in it, not outside the allocation.
    (tests/test_bc7_gpu.py::test_second_launch_hand_over_is_invisible checks the values with equal block counts.)"""
    import torch
    for k in ("CVTTMI_BC7_HARD_MIN", "CVTTMI_BC7_HARD_CAP", "CVTTMI_BC7_HARD_DIV"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CVTTMI_BC7_HARD_CAP", "4096")
    monkeypatch.setenv("CVTTMI_BC7_HARD_MIN", "2")
    own = api.Context(0)  # the settings are read when the context is created
    rcp = _rcp()
    own.set_rcp_table(rcp)
    lib, h = own._lib, own._h
    lib.cvttmi_bc7_hard_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    blocks = np.concatenate([content.mixed_ldr_blocks(777, 40), content.config_blocks(9, 256, 256)])
    n = VARIANT_BLOCKS
    key = ("stale", n)
    if key not in _EXPECTED:
        _EXPECTED[key] = oracle_lib.encode_bc7(blocks[:n], _opt_bytes(api.Options()), _opt_bytes(_PLAN), rcp, threads=8)
    exp = _EXPECTED[key]
    opt = api.Options()
    big = torch.from_numpy(blocks).cuda()
    first = own.encode_bc7(big, opt, _PLAN)
    handed, slots = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.cvttmi_bc7_hard_stats(h, ctypes.byref(handed), ctypes.byref(slots)) == 0
    assert slots.value == 4096 and handed.value > 0, (handed.value, slots.value)
    if punchthrough_between:
        own.encode_bc7(big, api.Options(flags=api.Flags.Default | api.Flags.BC7_RespectPunchThrough), _PLAN)
    what = "264 blocks after %d with a hand-over" % len(blocks)
    src, unchanged = guarded.device_input(blocks[:n], 64, what=what + ": input")
    out, check = guarded.device_buffer(n * 16, 16, poison, back=first.numel(), what=what)
    assert lib.cvttmi_encode_bc7_device(h, out.data_ptr(), src.data_ptr(), n, _addr(opt), _addr(_PLAN), None) == 0
    check(exp)
    unchanged()
    own.close()


# ---------------------------------------------------------------- host-pointer entries: any alignment

def _host_in(array, offset):
    """the bytes of `array` at byte `offset` of a guarded numpy allocation: (address, unchanged())"""
    data = _bytes(array)
    view, check = guarded.host_buffer(data.size, offset, 0x3C, what="host input")
    view[:] = data
    return view, (lambda: check(data))


HOST_BYTE_OFFSETS = (0, 1, 3)
HOST_ENCODERS = {
    "bc7": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc7(h, o, i, n, _addr(opt), _addr(_PLAN)),
    "bc1": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc1(h, o, i, n, _addr(opt)),
    "bc3": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc3(h, o, i, n, _addr(opt)),
    "etc2rgba": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_rgba(h, o, i, n, _addr(opt)),
    "bc6hu": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc6h(h, o, i, n, _addr(opt), 0),
    "r11s": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_alpha11(h, o, i, n, 1, _addr(opt)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
@pytest.mark.parametrize("name", list(HOST_ENCODERS))
def test_host_encoders_take_any_alignment(ctx, oracle_lib, name, poison):
    """The reference's PixelBlockU8 and output are byte arrays: numpy views at byte offsets 0, 1 and 3, guarded outputs"""
    lib, h = ctx._lib, ctx._h
    kind, in_bpb, out_bpb = ENCODERS[name][:3]
    blocks, exp = source_blocks(kind), expected_encoding(oracle_lib, name)
    opt = api.Options()
    for n in (8, 264):
        for in_off in HOST_BYTE_OFFSETS:
            for out_off in HOST_BYTE_OFFSETS:
                what = "host %s, %d blocks, input +%d, output +%d bytes" % (name, n, in_off, out_off)
                src, unchanged = _host_in(blocks[:n], in_off)
                out, check = guarded.host_buffer(n * out_bpb, out_off, poison, what=what)
                assert HOST_ENCODERS[name](lib, h, out.ctypes.data, src.ctypes.data, n, opt) == 0, (what, lib.cvttmi_last_error(h))
                check(exp[:n])
                unchanged()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", POISONS)
def test_host_decode_and_measure_take_any_alignment(ctx, poison):
    lib, h = ctx._lib, ctx._h
    for fmt in ("bc1", "bc7"):
        fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
        packed, dec = decode_case(fmt)
        for n in (8, 264):
            for in_off in HOST_BYTE_OFFSETS:
                for out_off in HOST_BYTE_OFFSETS:
                    what = "host decode %s, %d blocks, input +%d, output +%d bytes" % (fmt, n, in_off, out_off)
                    src, unchanged = _host_in(packed[:n], in_off)
                    out, check = guarded.host_buffer(n * tex, out_off, poison, what=what)
                    assert lib.cvttmi_decode(h, fid, out.ctypes.data, src.ctypes.data, n) == 0, (what, lib.cvttmi_last_error(h))
                    check(dec[:n])
                    unchanged()
    fmt = "bc1"
    fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
    packed, source = decode_case(fmt)[0], measure_source(fmt)
    for n in (8, 264):
        tot_exp, pb_exp = measure_case(fmt, n)
        for in_off in HOST_BYTE_OFFSETS:
            for out_off in HOST_BYTE_OFFSETS:
                what = "host measure %s, %d blocks, inputs +%d, outputs +%d bytes" % (fmt, n, in_off, out_off)
                bc, bc_same = _host_in(packed[:n], in_off)
                src, src_same = _host_in(source[:n], in_off)
                tot, tot_check = guarded.host_buffer(80, out_off, poison, what=what + ": totals")
                pb, pb_check = guarded.host_buffer(n * 4, out_off, poison, what=what + ": per-block values")
                rc = lib.cvttmi_measure_error(h, fid, bc.ctypes.data, src.ctypes.data, n, pb.ctypes.data, tot.ctypes.data)
                assert rc == 0, (what, lib.cvttmi_last_error(h))
                tot_check(tot_exp)
                pb_check(pb_exp)
                bc_same()
                src_same()


@pytest.mark.gpu
def test_host_bc1_second_chunk_of_one_group(ctx, oracle_lib):
    """2^17 + 8 blocks: the host pipeline's second chunk is a single group, at odd byte offsets on both sides"""
    lib, h = ctx._lib, ctx._h
    n = (1 << 17) + 8
    idx = np.arange(n) % FULL
    blocks, exp = source_blocks("ldr")[idx], expected_encoding(oracle_lib, "bc1")[idx]
    opt = api.Options()
    src, unchanged = _host_in(blocks, 3)
    out, check = guarded.host_buffer(n * 8, 1, 0xA5, what="host bc1, 2^17 + 8 blocks")
    assert lib.cvttmi_encode_bc1(h, out.ctypes.data, src.ctypes.data, n, _addr(opt)) == 0, lib.cvttmi_last_error(h)
    check(exp)
    unchanged()


# ---------------------------------------------------------------- the alignment rule is enforced before anything is queued

def _rejected(lib, h, rc, checks, what):
    assert rc == E_INVALID, (what, rc)
    assert b"misaligned" in lib.cvttmi_last_error(h), (what, lib.cvttmi_last_error(h))
    for c in checks:
        c.untouched()


def _forbidden(align):
    """byte offsets the rule forbids for a pointer that needs `align`: +1, and +4 / +8 where those break it"""
    return [d for d in (1, 4, 8) if d % align]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ENCODERS))
def test_misaligned_device_pointers_are_rejected_by_encoders(ctx, name):
    """a device pointer that is not aligned to min(block, 16) bytes: CVTTMI_E_INVALID, cvttmi_last_error says why, and the
    poisoned output is untouched (no kernel ever sees such a pointer)"""
    lib, h = ctx._lib, ctx._h
    kind, in_bpb, out_bpb, call, _, _ = ENCODERS[name]
    opt = api.Options()
    n = 8
    src, _ = guarded.device_input(source_blocks(kind)[:n], 0)
    out, check = guarded.device_buffer(n * out_bpb, 0, 0xA5)
    for d in _forbidden(min(out_bpb, 16)):
        _rejected(lib, h, call(lib, h, out.data_ptr() + d, src.data_ptr(), n, opt), [check], "%s output +%d" % (name, d))
    for d in _forbidden(min(in_bpb, 16)):
        _rejected(lib, h, call(lib, h, out.data_ptr(), src.data_ptr() + d, n, opt), [check], "%s input +%d" % (name, d))


@pytest.mark.gpu
def test_misaligned_device_pointers_are_rejected_by_the_other_entries(ctx):
    lib, h = ctx._lib, ctx._h
    n = 8
    for fmt in DECODE_FORMATS:
        fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
        bc, _ = guarded.device_input(decode_case(fmt)[0][:n], 0)
        src, _ = guarded.device_input(measure_source(fmt)[:n], 0)
        out, check = guarded.device_buffer(n * tex, 0, 0xA5)
        tot, tot_check = guarded.device_buffer(80, 0, 0xA5)
        pb, pb_check = guarded.device_buffer(n * 4, 0, 0xA5)
        all_checks = [check, tot_check, pb_check]
        for d in _forbidden(16):
            _rejected(lib, h, lib.cvttmi_decode_device(h, fid, out.data_ptr() + d, bc.data_ptr(), n, None), all_checks, "decode %s output +%d" % (fmt, d))
            _rejected(lib, h, lib.cvttmi_measure_error_device(h, fid, bc.data_ptr(), src.data_ptr() + d, n, pb.data_ptr(), tot.data_ptr(), None),
                      all_checks, "measure %s source +%d" % (fmt, d))
        for d in _forbidden(min(bpb, 16)):
            _rejected(lib, h, lib.cvttmi_decode_device(h, fid, out.data_ptr(), bc.data_ptr() + d, n, None), all_checks, "decode %s input +%d" % (fmt, d))
            _rejected(lib, h, lib.cvttmi_measure_error_device(h, fid, bc.data_ptr() + d, src.data_ptr(), n, pb.data_ptr(), tot.data_ptr(), None),
                      all_checks, "measure %s packed +%d" % (fmt, d))
        for d in (1, 2):
            _rejected(lib, h, lib.cvttmi_measure_error_device(h, fid, bc.data_ptr(), src.data_ptr(), n, pb.data_ptr() + d, tot.data_ptr(), None),
                      all_checks, "measure %s values +%d" % (fmt, d))
        for d in (1, 4):
            _rejected(lib, h, lib.cvttmi_measure_error_device(h, fid, bc.data_ptr(), src.data_ptr(), n, pb.data_ptr(), tot.data_ptr() + d, None),
                      all_checks, "measure %s totals +%d" % (fmt, d))
    # images: the texel size
    w, hh = 8, 8
    for hdr, fmt in ((False, "bc1"), (True, "bc6hu")):
        fid, bpb = api.TEXTURE_FORMATS[fmt][:2]
        texel = 8 if hdr else 4
        image, _ = guarded.device_input(make_image(w, hh, hdr), 0)
        bc, _ = guarded.device_input(decode_case(fmt)[0][:4], 0)
        tot, tot_check = guarded.device_buffer(80, 0, 0x5A)
        pb, pb_check = guarded.device_buffer(4 * 4, 0, 0x5A)
        blocks, blocks_check = guarded.device_buffer(8 * 16 * texel, 0, 0x5A)
        checks = [tot_check, pb_check, blocks_check]
        pix = 1 if hdr else 0
        for d in _forbidden(texel):
            _rejected(lib, h, lib.cvttmi_measure_image_error_device(h, fid, bc.data_ptr(), image.data_ptr() + d, w, hh, w * texel, pix, pb.data_ptr(),
                                                                    tot.data_ptr(), None), checks, "measure_image %s image +%d" % (fmt, d))
            _rejected(lib, h, lib.cvttmi_tile_image_device(h, blocks.data_ptr(), image.data_ptr() + d, w, hh, w * texel, pix, None), checks,
                      "tile image +%d" % d)
        for d in _forbidden(16):
            _rejected(lib, h, lib.cvttmi_tile_image_device(h, blocks.data_ptr() + d, image.data_ptr(), w, hh, w * texel, pix, None), checks,
                      "tile blocks +%d" % d)
        for d in _forbidden(min(bpb, 16)):
            _rejected(lib, h, lib.cvttmi_measure_image_error_device(h, fid, bc.data_ptr() + d, image.data_ptr(), w, hh, w * texel, pix, pb.data_ptr(),
                                                                    tot.data_ptr(), None), checks, "measure_image %s packed +%d" % (fmt, d))
        _rejected(lib, h, lib.cvttmi_measure_image_error_device(h, fid, bc.data_ptr(), image.data_ptr(), w, hh, w * texel, pix, pb.data_ptr() + 2,
                                                                tot.data_ptr(), None), checks, "measure_image values +2")
        _rejected(lib, h, lib.cvttmi_measure_image_error_device(h, fid, bc.data_ptr(), image.data_ptr(), w, hh, w * texel, pix, pb.data_ptr(),
                                                                tot.data_ptr() + 4, None), checks, "measure_image totals +4")
    for bpb in (8, 16):
        packed, _ = guarded.device_input(np.zeros((8, bpb), np.uint8), 0)
        out, check = guarded.device_buffer(2 * bpb, 0, 0xA5)
        for d in _forbidden(bpb):
            _rejected(lib, h, lib.cvttmi_compact_rows_device(h, out.data_ptr() + d, packed.data_ptr(), 8, 4, bpb, None), [check], "compact output +%d" % d)
            _rejected(lib, h, lib.cvttmi_compact_rows_device(h, out.data_ptr(), packed.data_ptr() + d, 8, 4, bpb, None), [check], "compact input +%d" % d)


# ---------------------------------------------------------------- the generic entries: one call, a format id

# ENCODERS name -> (CVTTMI_FMT_* id, the Options AllocETC2Data was given or None): the same encode through cvttmi_encode[_device]
GENERIC = {name: (api.TEXTURE_FORMATS["eac" if name == "etc2alpha" else name][0], None) for name in ENCODERS if not name.startswith("with_data")}
GENERIC.update(with_data_rgb=(4, _ALLOC_OPT), with_data_rgba=(5, _ALLOC_OPT), with_data_punchthrough=(13, _ALLOC_OPT))
assert sorted({fid for fid, _ in GENERIC.values()}) == list(range(17))
# 8: one group, a part-filled wave in every mapping; 264 = 16 * 16 + 8 = 4 * 64 + 8: ends inside a wave of the 16-blocks-per-wave
# mappings (BC7, BC6H) and inside a workgroup of the 64- and 256-lane ones
GENERIC_SIZES = (8, 264)


def _generic_args(name, opt):
    """(format id, options, plan, allocOptions) as cvttmi_encode[_device] takes them: the plan for BC7 alone"""
    fid, alloc = GENERIC[name]
    return fid, _addr(opt), (_addr(_PLAN) if name == "bc7" else None), (_addr(alloc) if alloc is not None else None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GENERIC))
def test_generic_device_entry_equals_the_named_one(ctx, name):
    """cvttmi_encode_device(format id) writes the bytes of the format's named *_device entry (held to the oracle above), all of
    them and none outside, with input and output 1 and 3 blocks into their allocations"""
    lib, h = ctx._lib, ctx._h
    kind, in_bpb, out_bpb, named, _, _ = ENCODERS[name]
    blocks, opt = source_blocks(kind), api.Options()
    fid, optp, planp, allocp = _generic_args(name, opt)
    for n in GENERIC_SIZES:
        for in_off, out_off in ((1, 3), (3, 1)):
            what = "generic %s (format %d), %d blocks, input +%d, output +%d blocks" % (name, fid, n, in_off, out_off)
            src, unchanged = guarded.device_input(blocks[:n], in_off * in_bpb, what=what + ": input")
            ref, ref_check = guarded.device_buffer(n * out_bpb, out_off * out_bpb, 0x5A, what=what + ": named entry")
            assert named(lib, h, ref.data_ptr(), src.data_ptr(), n, opt) == 0, (what, lib.cvttmi_last_error(h))
            exp = ref_check.payload()
            ref_check.no_poison_blocks(8)
            out, check = guarded.device_buffer(n * out_bpb, out_off * out_bpb, 0xA5, what=what)
            assert lib.cvttmi_encode_device(h, fid, out.data_ptr(), src.data_ptr(), n, optp, planp, allocp, None) == 0, (what, lib.cvttmi_last_error(h))
            check(exp)
            check.no_poison_blocks(8)
            unchanged()


GENERIC_HOST = {
    "bc7": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc7(h, o, i, n, _addr(opt), _addr(_PLAN)),
    "bc4s": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc4(h, o, i, n, _addr(opt), 1),
    "bc6hs": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_bc6h(h, o, i, n, _addr(opt), 1),
    "etc2rgba": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_rgba(h, o, i, n, _addr(opt)),
    "r11s": lambda lib, h, o, i, n, opt: lib.cvttmi_encode_etc2_alpha11(h, o, i, n, 1, _addr(opt)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GENERIC_HOST))
def test_generic_host_entry_equals_the_named_one(ctx, name):
    """cvttmi_encode on host pointers one byte into their allocations, 264 blocks, against the named host entry"""
    lib, h = ctx._lib, ctx._h
    kind, in_bpb, out_bpb = ENCODERS[name][:3]
    opt, n = api.Options(), 264
    fid, optp, planp, allocp = _generic_args(name, opt)
    what = "generic host %s (format %d), %d blocks, input and output +1 byte" % (name, fid, n)
    src, unchanged = _host_in(source_blocks(kind)[:n], 1)
    ref, ref_check = guarded.host_buffer(n * out_bpb, 1, 0x5A, what=what + ": named entry")
    assert GENERIC_HOST[name](lib, h, ref.ctypes.data, src.ctypes.data, n, opt) == 0, (what, lib.cvttmi_last_error(h))
    exp = ref_check.payload()
    ref_check.no_poison_blocks(8)
    out, check = guarded.host_buffer(n * out_bpb, 1, 0xA5, what=what)
    assert lib.cvttmi_encode(h, fid, out.ctypes.data, src.ctypes.data, n, optp, planp, allocp) == 0, (what, lib.cvttmi_last_error(h))
    check(exp)
    check.no_poison_blocks(8)
    unchanged()


@pytest.mark.gpu
def test_generic_entry_refusals(ctx):
    """what cvttmi_encode_device refuses with CVTTMI_E_INVALID before anything is queued: the poisoned output stays untouched"""
    lib, h = ctx._lib, ctx._h
    opt = api.Options()
    n = 16
    src, _ = guarded.device_input(source_blocks("ldr")[:n], 0)
    out, check = guarded.device_buffer(n * 16, 0, 0xA5)
    o, i, optp, planp = out.data_ptr(), src.data_ptr(), _addr(opt), _addr(_PLAN)
    bc7, bc1 = api.TEXTURE_FORMATS["bc7"][0], api.TEXTURE_FORMATS["bc1"][0]
    cases = [("format -1", (-1, o, i, 8, optp, planp, None, None), b"invalid argument"),
             ("format 17", (17, o, i, 8, optp, planp, None, None), b"invalid argument"),
             ("BC7 without a plan", (bc7, o, i, 8, optp, None, None, None), b"invalid argument"),
             ("BC7 without options", (bc7, o, i, 8, None, planp, None, None), b"invalid argument"),
             ("BC1 without options", (bc1, o, i, 8, None, None, None, None), b"invalid argument"),
             ("12 blocks", (bc1, o, i, 12, optp, None, None, None), b"invalid argument"),
             ("8-byte format, output +4", (bc1, o + 4, i, 8, optp, None, None, None), b"misaligned"),
             ("16-byte format, output +8", (bc7, o + 8, i, 8, optp, planp, None, None), b"misaligned"),
             ("16-byte format, input +8", (bc7, o, i + 8, 8, optp, planp, None, None), b"misaligned")]
    for what, args, text in cases:
        assert lib.cvttmi_encode_device(h, *args) == E_INVALID, what
        assert text in lib.cvttmi_last_error(h), (what, lib.cvttmi_last_error(h))
        check.untouched()
    assert lib.cvttmi_encode_device(None, bc1, o, i, 8, optp, None, None, None) == E_INVALID  # no context: no text to keep
    # the host entry: the same argument checks (host pointers need no alignment)
    hsrc, _ = _host_in(source_blocks("ldr")[:n], 0)
    hout, hcheck = guarded.host_buffer(n * 16, 0, 0xA5)
    ho, hi = hout.ctypes.data, hsrc.ctypes.data
    for what, args in (("format -1", (-1, ho, hi, 8, optp, planp, None)), ("format 17", (17, ho, hi, 8, optp, planp, None)),
                       ("BC7 without a plan", (bc7, ho, hi, 8, optp, None, None)), ("BC1 without options", (bc1, ho, hi, 8, None, None, None)),
                       ("12 blocks", (bc1, ho, hi, 12, optp, None, None))):
        assert lib.cvttmi_encode(h, *args) == E_INVALID, what
        assert b"invalid argument" in lib.cvttmi_last_error(h), (what, lib.cvttmi_last_error(h))
        hcheck.untouched()
    check.untouched()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["bc7", "bc6hu", "bc6hs"])
def test_named_decoders_equal_the_generic_one(ctx, fmt):
    """cvttmi_decode_bc7_device / cvttmi_decode_bc6h_device are cvttmi_decode_device with their id: the same bytes"""
    lib, h = ctx._lib, ctx._h
    fid, bpb, tex, _ = api.TEXTURE_FORMATS[fmt]
    packed = decode_case(fmt)[0]
    for n in GENERIC_SIZES:
        what = "decode %s, %d blocks" % (fmt, n)
        src, unchanged = guarded.device_input(packed[:n], bpb, what=what + ": input")
        ref, ref_check = guarded.device_buffer(n * tex, 3 * tex, 0x5A, what=what + ": generic entry")
        assert lib.cvttmi_decode_device(h, fid, ref.data_ptr(), src.data_ptr(), n, None) == 0, (what, lib.cvttmi_last_error(h))
        out, check = guarded.device_buffer(n * tex, 3 * tex, 0xA5, what=what + ": named entry")
        rc = (lib.cvttmi_decode_bc7_device(h, out.data_ptr(), src.data_ptr(), n, None) if fmt == "bc7"
              else lib.cvttmi_decode_bc6h_device(h, out.data_ptr(), src.data_ptr(), n, 1 if fmt == "bc6hs" else 0, None))
        assert rc == 0, (what, lib.cvttmi_last_error(h))
        check(ref_check.payload())
        check(_bytes(decode_case(fmt)[1]).reshape(FULL, tex)[:n])
        unchanged()
