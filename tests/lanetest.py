"""The lane-test library (tests/device/ -> convectionkernels_amd/lib/variants/libcvtt_lanetest.so) from Python: the table of its
sweeps, the ctypes plumbing (device memory comes from torch), the numpy restatements the integer and BC6H sweeps compare with,
and the source searches that keep the table honest.  The library compiles the product's own headers with the product's flags;
nothing here is part of the product."""
import concurrent.futures
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "convectionkernels_amd", "csrc")
LIB_PATH = os.path.join(ROOT, "convectionkernels_amd", "lib", "variants", "libcvtt_lanetest.so")

CHUNK = 4096          # tests/device/lanetest_checksum.h
CHUNKS = 1 << 20
HOST_THREADS = 16

# ---- the upper clamps the call sites pass --------------------------------------------------------------------------------
# (file, the text of the second argument) of every clampRound( / clampHigh( call under csrc/ -> the values that argument takes.
# tests/test_lane_primitives_cpu.py searches the sources: a call site that is not here fails it.
CLAMP_SITES = {
    "clampRound": {
        ("bc7_chain.h", "maxValue"): (3.0, 7.0, 15.0),            # md.indexBits = 2, 3, 4
        ("bc7_dual.h", "rgbMax"): (3.0, 7.0),                     # rgbPrec = 2, 3
        ("bc7_dual.h", "alphaMaxV"): (3.0, 7.0),
        ("bc1_kernel.hip", "maxValue"): (2.0, 3.0),               # range = 3, 4
        ("bc1_kernel.hip", "255.0f"): (255.0,),
        ("bc1_kernel.hip", "2047.0f"): (2047.0,),
        ("bc6h_kernel.hip", "maxValue"): (7.0, 15.0),             # indexBits = 3, 4
        ("bc6h_kernel.hip", "maxValueB"): (7.0, 15.0),
        ("s3tc_alpha_kernel.hip", "maxValue"): (5.0, 7.0),        # RANGE = 6, 8
        ("s3tc_alpha_kernel.hip", "255.0f"): (255.0,),
        ("s3tc_alpha_kernel.hip", "15.0f"): (15.0,),
        ("selftest_kernel.hip", "255.0f"): (255.0,),
    },
    "clampHigh": {
        ("bc7_dual.h", "rgbMax"): (3.0, 7.0),
        ("bc7_dual.h", "alphaMaxV"): (3.0, 7.0),
    },
}
# what the sweeps take whether or not a call site passes it today: 1 (a two-level index) with the common index ranges and the
# endpoint range for clampRound; 15 with 3 and 7 for the byte of clampHigh, the three tools/cvt_pk_u8_probe.hip was run for
CLAMP_EXTRA = {"clampRound": (1.0, 3.0, 7.0, 15.0, 255.0), "clampHigh": (3.0, 7.0, 15.0)}


def clamp_values(fn):
    vals = set(CLAMP_EXTRA[fn])
    for v in CLAMP_SITES[fn].values():
        vals |= set(v)
    return tuple(sorted(vals))


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def find_clamp_sites(fn):
    """{(file, second argument)} of the calls of `fn` in the sources under csrc/, definitions and comments left out"""
    found = set()
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".h", ".hip", ".cpp")):
            continue
        text = _strip_comments(open(os.path.join(CSRC, name)).read())
        for m in re.finditer(r"\b%s\(" % fn, text):
            if re.search(r"float\s+$", text[max(0, m.start() - 16):m.start()]):
                continue  # the definition
            depth, i, last_comma = 1, m.end(), None
            while depth:
                c = text[i]
                if c == "(":
                    depth += 1
                elif c == ")":
                    depth -= 1
                elif c == "," and depth == 1:
                    last_comma = i
                i += 1
            assert last_comma is not None, (name, text[m.start():i])
            found.add((name, text[last_comma + 1:i - 1].strip()))
    return found


def bc6h_mode_table():
    """the rows of k_bc6h_mode_info (csrc/bc6h_layout.h): [mode id, partitioned, transformed, aPrec, bPrec r, g, b]"""
    text = open(os.path.join(CSRC, "bc6h_layout.h")).read()
    body = re.search(r"k_bc6h_mode_info\[14\]\[7\]\s*=\s*\{(.*?)\};", text, re.S).group(1)
    rows = [[int(x, 0) for x in r.split(",")] for r in re.findall(r"\{([^{}]*)\}", body)]
    assert len(rows) == 14 and all(len(r) == 7 for r in rows)
    return rows


def bc6h_precisions():
    return sorted({r[3] for r in bc6h_mode_table()})


def bc6h_lost_bits():
    """16 - bPrec of every mode: what the kernel's mode words hold per channel, transformed or not"""
    return sorted({16 - b for r in bc6h_mode_table() for b in r[4:7]})


# ---- the library ---------------------------------------------------------------------------------------------------------
_lib = None


def load():
    global _lib
    if _lib is None:
        from convectionkernels_amd import api
        api.load_library()  # one HIP runtime per process: the product's loader maps the right one first
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing: build it with `make -C convectionkernels_amd/csrc`" % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
    return _lib


# The 2^32 sweeps: id -> (device symbol, hi or None, host reference symbol, its leading arguments).  The device symbol has a
# twin <symbol>_chunk.
def _sweeps32():
    t = {}
    for hi in clamp_values("clampRound"):
        t["clampRound(v, %g)" % hi] = ("lanetest_clamp_round", hi, "lanetest_ref_clamp_convert", (ctypes.c_float(hi), 0))
    for hi in clamp_values("clampHigh"):
        t["cvt_pk_u8(clampHigh(v, %g))" % hi] = ("lanetest_clamp_high_byte", hi, "lanetest_ref_clamp_convert", (ctypes.c_float(hi), 0))
    for hi in sorted({v for vals in CLAMP_SITES["clampHigh"].values() for v in vals}):
        t["roundClampLow(clampHigh(v, %g))" % hi] = ("lanetest_round_clamp_low", hi, "lanetest_ref_clamp_convert", (ctypes.c_float(hi), 1))
    t["endpointByte(v)"] = ("lanetest_endpoint_byte", None, "lanetest_ref_clamp_convert", (ctypes.c_float(255.0), 0))
    t["safeDenom(v)"] = ("lanetest_safe_denom", None, "lanetest_ref_safe_denom", ())
    t["plainByte<RGBA8>(s)"] = ("lanetest_plain_byte_u8", None, "lanetest_ref_plain_byte", (0,))
    t["plainByte<RGBA8_SNORM>(s)"] = ("lanetest_plain_byte_s8", None, "lanetest_ref_plain_byte", (1,))
    t["normalByte<RGBA8>(q)"] = ("lanetest_normal_byte_u8", None, "lanetest_ref_normal_byte", (0,))
    t["normalByte<RGBA8_SNORM>(q)"] = ("lanetest_normal_byte_s8", None, "lanetest_ref_normal_byte", (1,))
    return t


SWEEPS32 = _sweeps32()

# every other entry point of the library that a sweep calls
OTHER_SYMBOLS = (
    "lanetest_pair_ops", "lanetest_half_to_float", "lanetest_ceil_div31", "lanetest_quantize", "lanetest_unquantize", "lanetest_mul_u24",
    "lanetest_delta", "lanetest_tweak_of", "lanetest_reconstruct", "lanetest_channel_error", "lanetest_sub_byte_k",
    "lanetest_udiv_small", "lanetest_udiv_small20", "lanetest_min_loaded", "lanetest_lane_rows", "lanetest_lane_moves",
    "lanetest_wave_argmin", "lanetest_srgb_encode", "lanetest_box4x8", "lanetest_box4x8_inputs",
    "lanetest_ref_sse_min", "lanetest_ref_sse_max",
)


def all_symbols():
    names = set(OTHER_SYMBOLS)
    for dev, _hi, ref, _args in SWEEPS32.values():
        names |= {dev, dev + "_chunk", ref}
    return sorted(names)


# ---- host references of the 2^32 sweeps ------------------------------------------------------------------------------------
_host_sums = {}


def host_sums(ref, args):
    """the 2^20 chunk checksums of a host reference, on at most 16 threads; kept, since several sweeps share one reference"""
    key = (ref,) + tuple(getattr(a, "value", a) for a in args)
    if key not in _host_sums:
        fn = getattr(load(), ref)
        sums = np.empty(CHUNKS, np.uint64)
        workers = max(1, min(HOST_THREADS, os.cpu_count() or 1))
        per = CHUNKS // (workers * 4)
        starts = list(range(0, CHUNKS, per))

        def part(c0):
            n = min(per, CHUNKS - c0)
            rc = fn(*args, ctypes.c_uint32(c0), ctypes.c_uint32(n), ctypes.c_void_p(sums[c0:].ctypes.data), None)
            assert rc == 0, (ref, c0)

        with concurrent.futures.ThreadPoolExecutor(workers) as pool:
            list(pool.map(part, starts))
        _host_sums[key] = sums
    return _host_sums[key]


def host_chunk(ref, args, chunk):
    out = np.empty(CHUNK, np.uint32)
    assert getattr(load(), ref)(*args, ctypes.c_uint32(chunk), ctypes.c_uint32(1), None, ctypes.c_void_p(out.ctypes.data)) == 0
    return out


# ---- device plumbing -----------------------------------------------------------------------------------------------------
def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc, what):
    assert rc == 0, "%s: hipError %d" % (what, rc)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _empty(n, dtype):
    import torch
    return torch.empty(n, dtype=dtype, device="cuda:0")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def device_sums(dev, hi):
    import torch
    sums = _empty(CHUNKS, torch.int64)
    _check(getattr(load(), dev)(ctypes.c_float(hi or 0.0), ptr(sums), _stream()), dev)
    torch.cuda.synchronize()
    return _host(sums, np.uint64)


def device_chunk(dev, hi, chunk):
    import torch
    out = _empty(CHUNK, torch.int32)
    _check(getattr(load(), dev + "_chunk")(ctypes.c_float(hi or 0.0), ctypes.c_uint32(chunk), ptr(out), _stream()), dev + "_chunk")
    torch.cuda.synchronize()
    return _host(out, np.uint32)


def sweep32_mismatches(name, skip_chunks=(), entry=None):
    """None, or the failure message of the 2^32 sweep `name` (`entry`: a row that is not in the table): the count of mismatching
    inputs (exact while at most 64 chunks differ) and the lowest one, with both results"""
    dev, hi, ref, args = entry or SWEEPS32[name]
    want, got = host_sums(ref, args), device_sums(dev, hi)
    bad = np.flatnonzero(want != got)
    if len(skip_chunks):
        bad = np.setdiff1d(bad, np.asarray(skip_chunks))
    if len(bad) == 0:
        return None
    count, lowest = 0, None
    for c in bad[:64]:
        w, g = host_chunk(ref, args, int(c)), device_chunk(dev, hi, int(c))
        j = np.flatnonzero(w != g)
        count += len(j)
        if lowest is None and len(j):
            lowest = "0x%08x: the device gives 0x%x, the host 0x%x" % ((int(c) << 12) | int(j[0]), int(g[j[0]]), int(w[j[0]]))
    more = "" if len(bad) <= 64 else " in the first 64 of %d differing chunks" % len(bad)
    return "%s: %d of 2^32 inputs differ%s, the lowest %s" % (name, count, more, lowest)


def reduced(symbol, *args):
    """(mismatches, lowest input number) of a sweep that compares on the device"""
    import torch
    res = to_device(np.array([0, 0xffffffffffffffff], np.uint64).view(np.int64))
    _check(getattr(load(), symbol)(*args, ptr(res), _stream()), symbol)
    torch.cuda.synchronize()
    r = _host(res, np.uint64)
    return int(r[0]), int(r[1])


def mapped(symbol, inputs, outputs, extra=(), count=True):
    """symbol(inputs..., n, extra..., outputs..., stream) -> the outputs as int32 arrays.  `inputs`: equally long 4-byte arrays"""
    import torch
    n = len(inputs[0]) if inputs else None
    ins = [to_device(np.asarray(a).view(np.int32)) for a in inputs]
    outs = [_empty(o, torch.int32) for o in outputs]
    args = [ptr(t) for t in ins] + ([ctypes.c_uint32(n)] if count and n is not None else []) + list(extra) + [ptr(t) for t in outs]
    _check(getattr(load(), symbol)(*args, _stream()), symbol)
    torch.cuda.synchronize()
    return [_host(t, np.int32) for t in outs]


def first_difference(name, got, want, describe):
    """None, or "<name>: N of M inputs differ, the lowest <describe(i)>" """
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if len(bad) == 0:
        return None
    i = int(bad[0])
    return "%s: %d of %d inputs differ, the lowest %s: the device gives %s, expected %s" % (name, len(bad), got.size, describe(i), got.flat[i], want.flat[i])


# ---- numpy restatements ----------------------------------------------------------------------------------------------------
def div_round_up(a, b):
    """a / b in binary32 rounded toward +inf (tools/check_bc6h_quantize.py): the round-to-nearest quotient corrected by the sign
    of the exact residual"""
    a32, b32 = np.float32(a), np.float32(b)
    q = (a32 / b32).astype(np.float32)
    r = a32.astype(np.float64) - q.astype(np.float64) * np.float64(b)
    return np.where(r > 0, np.nextafter(q, np.float32(np.inf)), q).astype(np.float32)


def quantize_unsigned_ref(elem, precision):
    """QuantizeSingleEndpointElementUnsigned as the reference computes it: elem * 64 / 31 in binary32 rounded up, capped at 65535,
    minus 32768, the ceiling, the saturation to int16, re-biased; then the shift"""
    elem = np.asarray(elem, np.int64)
    v = np.minimum(div_round_up((elem * 64).astype(np.float32), 31.0), np.float32(65535.0))
    i = np.minimum(np.ceil((v - np.float32(32768.0)).astype(np.float32)).astype(np.int64), 32767)
    return ((i & 0xffff) ^ 0x8000) >> (16 - np.asarray(precision, np.int64))


def quantize_signed_ref(elem, precision):
    """QuantizeSingleEndpointElementSigned: |elem| * 32 / 31 in binary32 rounded up, the ceiling, saturated to int16, shifted, the
    sign put back"""
    elem = np.asarray(elem, np.int64)
    a = np.abs(elem)
    i = np.minimum(np.ceil(div_round_up((a * 32).astype(np.float32), 31.0)).astype(np.int64), 32767)
    q = i >> (16 - np.asarray(precision, np.int64))
    return np.where(elem < 0, -q, q)


def unquantize_unsigned_ref(comp, precision):
    comp, precision = np.asarray(comp, np.int64), np.asarray(precision, np.int64)
    shift = np.maximum(16 - precision, 0)
    unq = ((comp << shift) + (0x8000 >> precision)) & 0xffff
    unq = np.where(comp == 0, 0, unq)
    unq = np.where(comp > (1 << precision) - 2, 0xffff, unq)
    unq = np.where(precision < 15, unq, comp & 0xffff)
    return unq, (unq * 31) >> 6


def unquantize_signed_ref(comp, precision):
    comp, precision = np.asarray(comp, np.int64), np.asarray(precision, np.int64)
    neg, a = comp < 0, np.abs(comp)
    shift = np.maximum(16 - precision, 0)
    au = ((a << shift) + (0x4000 >> (precision - 1))) & 0xffff
    au = np.where(au >= 0x8000, au - 0x10000, au)  # the 16-bit lane as an int16
    au = np.where(comp == 0, 0, au)
    au = np.where(comp > (1 << (precision - 1)) - 2, 0x7fff, au)
    au = np.where(precision >= 16, a, au)
    unq = np.where(precision >= 16, comp, np.where(neg, -au, au))
    funq = np.minimum(((au & 0xffff) * 31) >> 5, 32767)
    return unq, np.where(neg, -funq, funq)


def half_to_float_ref(v16):
    """TwosCLHalfToFloat's bit manipulation on 16-bit patterns, the final subtraction in binary32: the float's bits"""
    v = np.asarray(v16, np.uint32) & 0xffff
    sign, mantissa, exponent = v & 0x8000, v & 0x03ff, v & 0x7c00
    denormal = exponent == 0
    exponent = ((exponent >> 3) + 14336) & 0xffff
    corr = np.where(denormal, sign | 14336, 0).astype(np.uint32)
    high = sign | exponent | (mantissa >> 3)
    low = (mantissa << 13) & 0xffff
    a = ((high << 16) | low).astype(np.uint32).view(np.float32)
    b = (corr << 16).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        return (a - b).astype(np.float32).view(np.uint32)


def delta_ref(v, base, lost, mask):
    """deltaOf: v - base in 16 bits, of which a transformed mode keeps the low 16 - lost, sign-extended; deltaFits: base + that
    delta gives v back in the bits of `mask`"""
    v, base, lost, mask = (np.asarray(x, np.int64) for x in (v, base, lost, mask))
    keep = 16 - lost
    d = (v - base) & ((1 << keep) - 1)
    d = np.where(d >> (keep - 1) != 0, d - (1 << keep), d)
    return d, (((d + base) & mask & 0xffff) == (v & mask & 0xffff)).astype(np.int64)


def normal_byte_ref(bits, snorm):
    """the two formulas of normalByte in binary32, the product, the sum and the floor rounded one by one; 0 outside |q| <= 1 + 2^-20"""
    bits = np.asarray(bits, np.uint32)
    q = bits.view(np.float32)
    inside = (bits & 0x7fffffff) <= 0x3f800008
    with np.errstate(all="ignore"):
        if snorm:
            s = ((q * np.float32(127.0)).astype(np.float32) + np.float32(0.5)).astype(np.float32)
            r = np.clip(np.floor(np.where(inside, s, 0)).astype(np.int64), -127, 127) & 255
        else:
            s = ((q * np.float32(127.5)).astype(np.float32) + np.float32(128.0)).astype(np.float32)
            r = np.clip(np.floor(np.where(inside, s, 0)).astype(np.int64), 0, 255)
    return np.where(inside, r, 0).astype(np.uint32)


def chunk_sums_ref(results):
    """the checksums of whole chunks of results (tests/device/lanetest_checksum.h)"""
    r = np.asarray(results, np.uint32).reshape(-1, CHUNK)
    j = np.arange(CHUNK, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (r ^ (j * np.uint64(0x9E3779B1)).astype(np.uint32)).astype(np.uint64)
        return (x * (np.uint64(0x9E3779B97F4A7C15) + np.uint64(2) * j)).sum(axis=1, dtype=np.uint64)


# the float edge set of the pair sweeps: +-0, +-denormal (smallest and largest), +-min normal, +-1, +-FLT_MAX, +-inf, quiet and
# signalling NaN of both signs
EDGE_BITS = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000, 0x3f800000, 0xbf800000,
                      0x7f7fffff, 0xff7fffff, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00000, 0x7fc12345, 0x7f800001],
                     np.uint32)


def float_pairs(seed, n):
    """n pseudo-random pairs of bit patterns, then every ordered pair of the edge set"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ea, eb = np.meshgrid(EDGE_BITS, EDGE_BITS, indexing="ij")
    return np.concatenate([a, ea.ravel()]), np.concatenate([b, eb.ravel()])


def host_pairs(ref, a, b):
    out = np.empty(len(a), np.uint32)
    getattr(load(), ref)(ctypes.c_void_p(a.ctypes.data), ctypes.c_void_p(b.ctypes.data), ctypes.c_uint32(len(a)), ctypes.c_void_p(out.ctypes.data))
    return out
