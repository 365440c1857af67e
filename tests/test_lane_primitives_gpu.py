"""Every lane primitive's exactness claim, swept on the device over its whole domain (tests/device/, tests/lanetest.py).  The
kernels under test are the product's own headers compiled with the product's flags into a library of their own; the expected
values are exact -- the SSE2 instruction a primitive stands for, computed on the host; the plain integer form; a numpy
restatement of the reference's sequence -- so every comparison is for equality.  A failure names the primitive, the count of
mismatches and the lowest mismatching input."""
import ctypes

import numpy as np
import pytest

import lanetest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lt(gpu_ctx):
    return lanetest.load()


# ---- float lane operations against SSE2, all 2^32 patterns ------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in lanetest.SWEEPS32 if not n.startswith(("plainByte", "normalByte"))])
def test_float_lane_op_equals_sse2_on_every_bit_pattern(lt, name):
    msg = lanetest.sweep32_mismatches(name)
    assert msg is None, msg


def test_sweep_reports_the_lowest_input_of_a_wrong_pairing(lt):
    """the machinery itself: clampRound(v, 3) held against the host sequence at hi = 7 must name 3.5, the lowest pattern that
    rounds above 3, with both values"""
    msg = lanetest.sweep32_mismatches("clampRound(v, 3) against hi = 7", entry=("lanetest_clamp_round", 3.0, "lanetest_ref_clamp_convert", (ctypes.c_float(7.0), 0)))
    assert msg is not None and "the lowest 0x40600000: the device gives 0x3, the host 0x4" in msg, msg


@pytest.fixture(scope="module")
def pairs():
    return lanetest.float_pairs(20240611, 1 << 24)


def _pair_text(a, b):
    return lambda i: "(0x%08x, 0x%08x)" % (a[i], b[i])


def test_sse_min_max_equal_minss_maxss(lt, pairs):
    a, b = pairs
    got_min, got_max = lanetest.mapped("lanetest_pair_ops", [a, b], [len(a), len(a)])
    for name, got, ref in (("sseMin", got_min, "lanetest_ref_sse_min"), ("sseMax", got_max, "lanetest_ref_sse_max")):
        msg = lanetest.first_difference(name, got.view(np.uint32), lanetest.host_pairs(ref, a, b), _pair_text(a, b))
        assert msg is None, msg


def test_min_loaded_is_the_smaller_value(lt, pairs):
    """its stated precondition: no NaN, no -0"""
    a, b = pairs
    ok = np.ones(len(a), bool)
    for x in (a, b):
        ok &= ((x & 0x7fffffff) <= 0x7f800000) & (x != 0x80000000)
    a, b = a[ok], b[ok]
    got, = lanetest.mapped("lanetest_min_loaded", [a, b], [len(a)])
    want = np.where(a.view(np.float32) <= b.view(np.float32), a, b)
    msg = lanetest.first_difference("minLoaded", got.view(np.uint32), want, _pair_text(a, b))
    assert msg is None, msg


def test_twos_cl_half_to_float_on_every_pattern(lt):
    """<true> is the bit manipulation itself on all 65 536 patterns.  <false> takes the hardware conversion and is claimed for the
    finite non-negative patterns (bc6h_quant.h: inputs are clamped to [0, 0x7BFF]); there it must equal the same restatement,
    and it is held on the finite negative patterns too.  Its true domain ends there (measured on the MI355X):
      * 0x8000, the negative zero: the conversion keeps the sign (-0), the bit manipulation subtracts two equal numbers (+0);
      * exponent field 31, the infinities and NaNs of binary16: the conversion gives infinities and NaNs, the bit manipulation
        65536 ... 131008.
    The unsigned format reaches neither -- no negative pattern at all -- so they are outside the claim and not compared."""
    got_u, got_s = lanetest.mapped("lanetest_half_to_float", [], [65536, 65536])
    v = np.arange(65536, dtype=np.uint32)
    want = lanetest.half_to_float_ref(v)
    msg = lanetest.first_difference("twosCLHalfToFloat<true>", got_s.view(np.uint32), want, lambda i: "0x%04x" % i)
    assert msg is None, msg
    finite = ((v & 0x7c00) != 0x7c00) & (v != 0x8000)
    assert finite[:0x7c00].all()  # the claim, whole
    msg = lanetest.first_difference("twosCLHalfToFloat<false>", got_u.view(np.uint32)[finite], want[finite], lambda i: "0x%04x" % v[finite][i])
    assert msg is None, msg


@pytest.mark.parametrize("name", [n for n in lanetest.SWEEPS32 if n.startswith("normalByte")])
def test_normal_byte_on_every_unit_component(lt, name):
    msg = lanetest.sweep32_mismatches(name)
    assert msg is None, msg


# ---- integer claims against the plain form ----------------------------------------------------------------------------------
def test_udiv_small_is_the_integer_quotient(lt):
    n, first = lanetest.reduced("lanetest_udiv_small")
    assert n == 0, "udivSmall: %d of 2^16 x 4095 inputs differ, the lowest n = %d, d = %d" % (n, first & 0xffff, first >> 16)


def test_udiv_small20_is_the_ceiling(lt):
    got, = lanetest.mapped("lanetest_udiv_small20", [], [128])
    d = np.arange(1, 129)
    msg = lanetest.first_difference("udivSmall20", got, -((-1 << 20) // d), lambda i: "d = %d" % d[i])
    assert msg is None, msg


def ceil_div31_domain():
    """The n below which ceilDiv31 is exact.  With x = n + 30 = 31 q + r the product x * 2216757579 / 2^36 is q + r / 31 + x * 8213 /
    (31 * 2^36), and its floor stays q while r / 31 plus the last term stays below 1: x * 8213 < (31 - r) * 2^36.  r = 30 binds first:
    the lowest x = 30 (mod 31) with x * 8213 >= 2^36."""
    x = -(-(1 << 36) // 8213)
    x += (30 - x) % 31
    return x - 30


def test_ceil_div31(lt):
    """bc6h_quant.h gives the domain as 0 <= n < 2^23 and, in the same comment, as x = n + 30 < 8.3 million.  The second is the true
    one: exact for n < 8 367 148 (the derivation above), and on the MI355X 693 of the n from there to 2^23 come out one too high, the
    lowest n = 8 367 148 itself.  The callers pass elem * 64 and |elem| * 32 with elem <= 31743, at most 2 031 552."""
    n = ceil_div31_domain()
    assert n == 8367148 and 31743 * 64 < n <= 1 << 23
    got, = lanetest.mapped("lanetest_ceil_div31", [], [n], extra=(ctypes.c_uint32(n),))
    msg = lanetest.first_difference("ceilDiv31", got, (np.arange(n, dtype=np.int64) + 30) // 31, lambda i: "n = %d" % i)
    assert msg is None, msg


def _grid(*axes):
    return [g.ravel().astype(np.int32) for g in np.meshgrid(*axes, indexing="ij")]


def test_bc6h_quantize_equals_the_float_sequence(lt):
    prec = lanetest.bc6h_precisions()
    elem, p = _grid(np.arange(0, 31744), prec)
    got, = lanetest.mapped("lanetest_quantize", [elem, p], [len(elem)], extra=(0,))
    msg = lanetest.first_difference("quantizeUnsigned", got, lanetest.quantize_unsigned_ref(elem, p), lambda i: "elem = %d, precision = %d" % (elem[i], p[i]))
    assert msg is None, msg
    elem, p = _grid(np.arange(-31743, 31744), prec)
    got, = lanetest.mapped("lanetest_quantize", [elem, p], [len(elem)], extra=(1,))
    msg = lanetest.first_difference("quantizeSigned", got, lanetest.quantize_signed_ref(elem, p), lambda i: "elem = %d, precision = %d" % (elem[i], p[i]))
    assert msg is None, msg


def test_bc6h_unquantize(lt):
    for signed, ref in ((0, lanetest.unquantize_unsigned_ref), (1, lanetest.unquantize_signed_ref)):
        comp = np.concatenate([np.arange(-(1 << (p - 1)) + 1, 1 << (p - 1)) if signed else np.arange(0, 1 << p) for p in lanetest.bc6h_precisions()])
        p = np.concatenate([np.full((1 << p) - 1 if signed else 1 << p, p) for p in lanetest.bc6h_precisions()])
        comp, p = comp.astype(np.int32), p.astype(np.int32)
        got_unq, got_fin = lanetest.mapped("lanetest_unquantize", [comp, p], [len(comp), len(comp)], extra=(signed,))
        want_unq, want_fin = ref(comp, p)
        for what, got, want in (("unquantized", got_unq, want_unq), ("finished", got_fin, want_fin)):
            msg = lanetest.first_difference("unquantize%s, %s" % ("Signed" if signed else "Unsigned", what), got, want,
                                            lambda i: "comp = %d, precision = %d" % (comp[i], p[i]))
            assert msg is None, msg


def _sixteen_bit_points(lo):
    """lo ... lo + 65535 on a stride of 257, plus the 64 values nearest each end, around 0 and around the sign change"""
    pts = set(range(lo, lo + 65536, 257))
    for centre in (lo, lo + 65535, 0, 32768, -32768 if lo < 0 else 32768):
        pts |= {x for x in range(centre - 64, centre + 65) if lo <= x <= lo + 65535}
    return np.array(sorted(pts), np.int32)


WEIGHTS = np.array(sorted({0, 9, 18, 27, 37, 46, 55, 64} | {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64}), np.int32)


@pytest.mark.parametrize("variant,name,signed", [(0, "reconstructFrom<false, true>", False), (1, "reconstructFrom<false, false>", False),
                                                  (2, "reconstructFrom<true, true>", True), (3, "reconstructFrom<true, false>", True),
                                                  (4, "reconstructChannel<false>", False), (5, "reconstructChannel<true>", True)])
def test_bc6h_reconstruct_equals_two_multiplications(lt, variant, name, signed):
    e1 = _sixteen_bit_points(-32768 if signed else 0)
    d_e1, d_w = lanetest.to_device(e1), lanetest.to_device(WEIGHTS)
    n, first = lanetest.reduced("lanetest_reconstruct", variant, lanetest.ptr(d_e1), ctypes.c_uint32(len(e1)), lanetest.ptr(d_w), ctypes.c_uint32(len(WEIGHTS)))
    assert n == 0, "%s: %d of %d inputs differ, the lowest e0 = %d, e1 = %d, weight = %d" % (
        name, n, 65536 * len(e1) * len(WEIGHTS), (first >> 32) - (32768 if signed else 0), e1[(first >> 8) & 0xffffff], WEIGHTS[first & 0xff])


def test_mul_u24(lt):
    rng = np.random.default_rng(24)
    corners = np.array([0, 1, 2, 31, 64, 0x7fffff, 0x800000, 0xfffffe, 0xffffff], np.uint32)
    ca, cb = np.meshgrid(corners, corners, indexing="ij")
    a = np.concatenate([rng.integers(0, 1 << 24, 1 << 24, dtype=np.uint32), ca.ravel()])
    b = np.concatenate([rng.integers(0, 1 << 24, 1 << 24, dtype=np.uint32), cb.ravel()])
    got, = lanetest.mapped("lanetest_mul_u24", [a, b], [len(a)])
    want = ((a.astype(np.uint64) * b.astype(np.uint64)) & 0xffffffff).astype(np.uint32)
    msg = lanetest.first_difference("mulU24", got.view(np.uint32), want, lambda i: "(%d, %d)" % (a[i], b[i]))
    assert msg is None, msg


@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_bc7_channel_error_step(lt, channel):
    """madI24, subByte1<CH>, channelError<CH> and accumulateChannelError<CH> on the words bc7_chain.h forms: every pair of end point
    bytes, every weight 0 ... 64, every pixel byte"""
    n, first = lanetest.reduced("lanetest_channel_error", channel)
    assert n == 0, "madI24 / subByte1<%d> / channelError / accumulateChannelError: %d of 2^16 x 65 x 256 inputs differ, the lowest e0 = %d, e1 = %d, weight = %d, pixel byte = %d" % (
        channel, n, first >> 24, (first >> 16) & 255, (first >> 8) & 255, first & 255)


def test_sub_byte_k(lt):
    n, first = lanetest.reduced("lanetest_sub_byte_k")
    assert n == 0, "subByteK<K, CH>: %d of 12 x 2^16 inputs differ, the lowest K = %d, CH = %d, bytes %d and %d" % (
        n, (first >> 16) // 4, (first >> 16) % 4, (first >> 8) & 255, first & 255)


def test_bc6h_delta_of_and_delta_fits(lt):
    pts = np.unique(np.concatenate([_sixteen_bit_points(0), _sixteen_bit_points(-32768)]))
    pts = pts[::2] if len(pts) > 700 else pts
    pts = np.unique(np.concatenate([pts, [-32768, -32767, -1, 0, 1, 32767, 32768, 65535]])).astype(np.int32)
    masks = np.array([(1 << p) - 1 for p in lanetest.bc6h_precisions()], np.int32)
    lost = np.array(lanetest.bc6h_lost_bits(), np.int32)
    for m in masks:
        v, base, lo = _grid(pts, pts, lost)
        mk = np.full(len(v), m, np.int32)
        got_d, got_f = lanetest.mapped("lanetest_delta", [v, base, lo, mk], [len(v), len(v)])
        want_d, want_f = lanetest.delta_ref(v, base, lo, mk)
        text = lambda i: "v = %d, base = %d, lost bits = %d, mask = 0x%x" % (v[i], base[i], lo[i], m)
        for name, got, want in (("deltaOf", got_d, want_d), ("deltaFits", got_f, want_f)):
            msg = lanetest.first_difference(name, got, want, text)
            assert msg is None, msg


def test_tweak_of(lt):
    got, = lanetest.mapped("lanetest_tweak_of", [], [12])
    msg = lanetest.first_difference("tweakOf", got, np.arange(12) // 3, lambda i: "m = %d" % i)
    assert msg is None, msg


def test_srgb_encode_counts_the_thresholds(lt):
    from convectionkernels_amd import api
    _, thresholds = api.srgb_tables()
    n = 4 * 65535 + 1
    full, split = lanetest.mapped("lanetest_srgb_encode", [], [n, n], extra=(ctypes.c_uint32(n),))
    want = np.searchsorted(np.asarray(thresholds, np.int64), np.arange(n), side="right")  # the number of k with S >= U[k]
    for name, got in (("srgbEncode(SrgbTables)", full), ("srgbEncode(SrgbEncodeTables)", split)):
        msg = lanetest.first_difference(name, got, want, lambda i: "S = %d" % i)
        assert msg is None, msg


@pytest.mark.parametrize("name", [n for n in lanetest.SWEEPS32 if n.startswith("plainByte")])
def test_plain_byte_on_every_sum(lt, name):
    """For s > 2^31 - 2^17 - 1 the function's first step, s + 2^17, overflows an int -- no defined result -- so the last 32 chunks
    of the positive half are outside its domain and not compared; every other sum is"""
    outside = np.arange((1 << 19) - 32, 1 << 19)
    msg = lanetest.sweep32_mismatches(name, skip_chunks=outside)
    assert msg is None, msg


@pytest.mark.parametrize("kind,name", [(0, "box4x8<RGBA8>"), (2, "box4x8<RGBA8_SNORM>")])
def test_box4x8_equals_the_rule_byte_by_byte(lt, kind, name):
    seed, count = 0x5eed0000 + kind, 1296 + (1 << 26)
    n, first = lanetest.reduced("lanetest_box4x8", kind, ctypes.c_uint64(seed), ctypes.c_uint32(count))
    if n:
        words, = lanetest.mapped("lanetest_box4x8_inputs", [], [4], extra=(ctypes.c_uint64(seed), ctypes.c_uint32(first)))
        assert False, "%s: %d of %d quadruples differ, the lowest number %d: %s" % (name, n, count, first, ["0x%08x" % w for w in words.view(np.uint32)])


# ---- cross-lane primitives, one wave ------------------------------------------------------------------------------------------
def _lane_moves_expected(v, pick, with_min):
    lanes = np.arange(64)
    rows = {}
    for r in range(6):
        x = v[lanes ^ (1 << r)]
        for base in (0, 6, 12, 18, 24):
            rows[base + r] = x
    rows[30], rows[31] = v[lanes ^ 1], v[lanes ^ 2]
    for q in range(4):
        rows[32 + q] = v[(lanes & ~3) | q]
    quads = v.reshape(16, 4)
    rows[36] = np.repeat(np.bitwise_or.reduce(quads, axis=1), 4)
    if with_min:
        rows[37] = np.repeat(quads.view(np.float32).min(axis=1).view(np.uint32), 4)
    ballot = sum(int(b) << i for i, b in enumerate(v & 1))
    halves = np.where(lanes < 32, ballot & 0xffffffff, ballot >> 32)
    rows[38], rows[39] = halves, halves ^ 0xffffffff
    for r in (40, 41, 42):
        rows[r] = np.full(64, v[0])
    rows[43] = rows[44] = np.full(64, v[pick])
    return rows


ROW_NAMES = ([(r, "xorLane(int, %d)" % (1 << r)) for r in range(6)] + [(6 + r, "xorLaneI<%d>" % (1 << r)) for r in range(6)] +
             [(12 + r, "xorLaneF<%d>" % (1 << r)) for r in range(6)] + [(18 + r, "xorLane(float, %d)" % (1 << r)) for r in range(6)] +
             [(24 + r, "xorLane(unsigned, %d)" % (1 << r)) for r in range(6)] +
             [(30, "quadPerm<0xb1>"), (31, "quadPerm<0x4e>"), (32, "quadBcast<0>"), (33, "quadBcast<1>"), (34, "quadBcast<2>"), (35, "quadBcast<3>"),
              (36, "quadOr"), (37, "quadMin"), (38, "groupBits(ballot)"), (39, "groupBits(~ballot)"), (40, "uniU"), (41, "uniI"), (42, "uniF"),
              (43, "laneI"), (44, "laneF")])


def test_lane_moves(lt):
    rows = lt.lanetest_lane_rows()
    assert rows == len(ROW_NAMES)
    rng = np.random.default_rng(64)
    for case in range(16):
        finite = case % 2 == 1  # quadMin is compared on finite floats that differ within a quad; the moves on any bits
        if finite:
            v = rng.permutation(1 << 16)[:64].astype(np.uint32) * np.uint32(8191) + np.uint32(0x30000000 if case % 4 == 1 else 0xb0000000)
        else:
            v = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32)
        if case == 0:
            v = np.arange(64, dtype=np.uint32)  # every lane its own number
        pick = int(rng.integers(0, 64)) if case else 63
        got, = lanetest.mapped("lanetest_lane_moves", [v], [rows * 64], extra=(pick,), count=False)
        got = got.view(np.uint32).reshape(rows, 64)
        want = _lane_moves_expected(v, pick, finite)
        for r, name in ROW_NAMES:
            if r in want:
                msg = lanetest.first_difference(name, got[r], want[r].astype(np.uint32), lambda i: "lane %d of case %d" % (i, case))
                assert msg is None, msg


def _argmin_cases():
    """4096 cases of 64 (err, id): the ids distinct, not the lane numbers and in no order"""
    rng = np.random.default_rng(4096)
    flt_max = np.float32(np.finfo(np.float32).max)
    err = (rng.random((4096, 64), dtype=np.float32) * np.float32(1e6)).astype(np.float32) ** 2
    ids = (rng.permuted(np.tile(np.arange(64), (4096, 1)), axis=1) * 37 + 5 + 1000 * np.arange(4096)[:, None]).astype(np.int32)
    for c in range(4096):
        kind = c % 16
        lanes = rng.permutation(64)
        if kind in (1, 2):      # a tie among 2, 3 lanes at the minimum
            err[c, lanes[:kind + 1]] = err[c].min()
        elif kind == 3:         # a tie among all 64
            err[c, :] = err[c, 0]
        elif kind == 4:         # every lane FLT_MAX
            err[c, :] = flt_max
        elif kind == 5:         # +inf among finite values
            err[c, lanes[:rng.integers(1, 8)]] = np.inf
        elif kind == 6:         # one lane NaN
            err[c, lanes[0]] = np.nan
        elif kind == 7:         # several lanes NaN, one of them where the minimum was
            err[c, err[c].argmin()] = np.nan
            err[c, lanes[:rng.integers(2, 40)]] = np.nan
        elif kind == 8:         # all lanes NaN
            err[c, :] = np.nan
        elif kind == 9:         # FLT_MAX in most lanes, NaN in the rest: every lane ties
            err[c, :] = flt_max
            err[c, lanes[:5]] = np.nan
        elif kind == 10:        # zeros: a tie at +0
            err[c, lanes[:3]] = 0.0
    return err, ids


def test_wave_argmin(lt):
    err, ids = _argmin_cases()
    got_err, got_id = lanetest.mapped("lanetest_wave_argmin", [err.ravel(), ids.ravel()], [err.size, err.size], extra=(ctypes.c_uint32(4096),), count=False)
    counted = np.where(np.isnan(err), np.float32(np.finfo(np.float32).max), err)  # a NaN counts as FLT_MAX
    m = counted.min(axis=1)
    winner = np.where(counted == m[:, None], ids, np.iinfo(np.int32).max).min(axis=1)  # ties: the lowest id
    text = lambda i: "lane %d of case %d (kind %d)" % (i % 64, i // 64, (i // 64) % 16)
    msg = lanetest.first_difference("waveArgmin, the error", got_err.view(np.uint32), np.repeat(m.view(np.uint32), 64), text)
    assert msg is None, msg
    msg = lanetest.first_difference("waveArgmin, the id", got_id, np.repeat(winner, 64), text)
    assert msg is None, msg
