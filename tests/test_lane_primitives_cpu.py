"""What the lane-primitive sweeps (tests/test_lane_primitives_gpu.py) rest on, checked without a device: the lane-test library
was built and exports every entry point the table names, the SSE2 host references behave as the header comments say the
instructions do, the numpy restatements agree with tools/check_bc6h_quantize.py's float sequence and with the host references,
and the table's upper clamps are the ones the sources pass."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import lanetest

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_library_is_built_and_exports_every_sweep():
    assert os.path.exists(lanetest.LIB_PATH), "the default build makes libcvtt_lanetest.so (csrc/Makefile)"
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not installed")
    out = subprocess.check_output([READELF, "--dyn-syms", "--wide", lanetest.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " FUNC " in line and " GLOBAL " in line and " UND " not in line}
    missing = [s for s in lanetest.all_symbols() if s not in exported]
    assert not missing, missing
    lib = lanetest.load()
    for s in lanetest.all_symbols():
        assert hasattr(lib, s), s


def test_product_library_carries_none_of_it():
    from convectionkernels_amd import api
    lib = api.load_library()
    for s in lanetest.all_symbols():
        assert not hasattr(lib, s), s


def _clamp_convert(hi, bits, as_float=0):
    """the host reference on single patterns: the chunk that holds each of them"""
    out = []
    for b in bits:
        full = lanetest.host_chunk("lanetest_ref_clamp_convert", (ctypes.c_float(hi), as_float), int(b) >> 12)
        out.append(int(full[int(b) & 4095]))
    return out


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


@pytest.mark.parametrize("hi", lanetest.clamp_values("clampRound"))
def test_sse2_clamp_convert_on_the_edges(hi):
    nans = [0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00000, 0x7f800001, 0xffffffff]
    assert _clamp_convert(hi, nans) == [int(hi)] * len(nans)                      # MINPS hands a NaN's place to hi
    assert _clamp_convert(hi, [0x80000000, 0x00000000, _bits(-0.25), _bits(-1e30), 0xff800000, 0x80000001]) == [0] * 6
    assert _clamp_convert(hi, [0x80000000], as_float=1) == [0]                    # and the float of it is +0
    assert _clamp_convert(hi, [0x7f800000, _bits(hi), _bits(hi + 0.75), 0x7f7fffff]) == [int(hi)] * 4
    halves = [k + 0.5 for k in range(int(min(hi, 16)))]                           # halfway cases go to even
    assert _clamp_convert(hi, [_bits(h) for h in halves]) == [int(h + 0.5) & ~1 if int(h + 0.5) <= hi else int(hi) for h in halves]
    assert _clamp_convert(hi, [_bits(0.5), _bits(np.nextafter(np.float32(0.5), np.float32(1))), _bits(np.nextafter(np.float32(0.5), np.float32(0)))]) == [0, 1, 0]


def test_sse2_min_max_keep_the_second_operand():
    a, b = np.meshgrid(lanetest.EDGE_BITS, lanetest.EDGE_BITS, indexing="ij")
    a, b = a.ravel().copy(), b.ravel().copy()
    mn, mx = lanetest.host_pairs("lanetest_ref_sse_min", a, b), lanetest.host_pairs("lanetest_ref_sse_max", a, b)
    fa, fb = a.view(np.float32), b.view(np.float32)
    nan = np.isnan(fa) | np.isnan(fb)
    assert (mn[nan] == b[nan]).all() and (mx[nan] == b[nan]).all()              # b on NaN, either side
    zeros = ((a & 0x7fffffff) == 0) & ((b & 0x7fffffff) == 0)
    assert zeros.sum() == 4 and (mn[zeros] == b[zeros]).all() and (mx[zeros] == b[zeros]).all()  # b on equal zeros of either sign
    with np.errstate(invalid="ignore"):
        assert (mn[~nan] == np.where(fa < fb, a, b)[~nan]).all() and (mx[~nan] == np.where(fa > fb, a, b)[~nan]).all()


def test_quantize_restatements_agree_with_the_tool():
    """tools/check_bc6h_quantize.py asserts its float sequence against ceil(elem * 64 / 31) and ceil(elem * 32 / 31) at import; the
    restatements here are that sequence with the shift by the precision, so at precision 16 they must give those integers"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_bc6h_quantize", os.path.join(lanetest.ROOT, "tools", "check_bc6h_quantize.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    elem = np.arange(0, 31744)
    assert np.array_equal(lanetest.quantize_unsigned_ref(elem, 16), tool.c)
    assert np.array_equal(lanetest.quantize_signed_ref(elem, 16), np.minimum(tool.c2, 32767))
    assert np.array_equal(lanetest.quantize_signed_ref(-elem, 16), -np.minimum(tool.c2, 32767))
    assert np.array_equal(lanetest.div_round_up(np.float32(7.0), 31.0), tool.div_round_up(np.float32(7.0), 31.0))
    for p in lanetest.bc6h_precisions():
        assert np.array_equal(lanetest.quantize_unsigned_ref(elem, p), tool.c >> (16 - p))
        # unquantising what was quantised stays inside 16 bits and keeps the order
        unq, fin = lanetest.unquantize_unsigned_ref(np.arange(1 << p), p)
        assert unq[0] == 0 and unq[-1] == 0xffff and (np.diff(unq) > 0).all() and fin.max() == (0xffff * 31) >> 6
        unq, fin = lanetest.unquantize_signed_ref(np.arange(-(1 << (p - 1)) + 1, 1 << (p - 1)), p)
        # (the reference lifts only the largest POSITIVE component to 0x7fff: the ends are not mirror images, the rest is)
        assert (np.diff(unq) > 0).all() and unq.max() == 0x7fff and np.array_equal(unq[1:-1], -unq[-2:0:-1]) and np.array_equal(fin[1:-1], -fin[-2:0:-1])


def test_half_restatement_is_the_conversion_on_normal_halves():
    v = np.arange(65536, dtype=np.uint32)
    got = lanetest.half_to_float_ref(v).view(np.float32)
    want = v.astype(np.uint16).view(np.float16).astype(np.float32)
    normal = ((v & 0x7c00) != 0) & ((v & 0x7c00) != 0x7c00)
    assert np.array_equal(got[normal], want[normal])
    denormal = (v & 0x7c00) == 0
    assert np.array_equal(got[denormal], want[denormal] * np.float32(0.5))       # it halves them (bc6h_quant.h)


def test_bc6h_tables_read_from_the_source():
    assert lanetest.bc6h_precisions() == [6, 7, 8, 9, 10, 11, 12, 16]
    assert lanetest.bc6h_lost_bits() == [6, 7, 8, 10, 11, 12]


@pytest.mark.parametrize("snorm", [0, 1])
def test_normal_byte_host_reference_is_the_numpy_restatement(snorm):
    """the sweep compares with the host restatement in C++ (2^31 values in numpy take a minute); here the two restatements meet on
    the chunks around every edge of the domain and on a spread of others, results and checksums"""
    chunks = sorted({0, 1, 0x3f000, 0x3f7ff, 0x3f800, 0x3f801, 0x80000, 0x80001, 0xbf000, 0xbf7ff, 0xbf800, 0xbf801, 0x7f800, 0xfffff} |
                    set(range(0x30000, 0x3f800, 0x173)) | set(range(0xb0000, 0xbf800, 0x173)))
    lib = lanetest.load()
    for c in chunks:
        full, sums = np.empty(lanetest.CHUNK, np.uint32), np.empty(1, np.uint64)
        assert lib.lanetest_ref_normal_byte(snorm, ctypes.c_uint32(c), ctypes.c_uint32(1), ctypes.c_void_p(sums.ctypes.data), ctypes.c_void_p(full.ctypes.data)) == 0
        bits = (np.uint32(c) << np.uint32(12)) | np.arange(lanetest.CHUNK, dtype=np.uint32)
        want = lanetest.normal_byte_ref(bits, snorm)
        assert np.array_equal(full, want), "chunk 0x%x" % c
        assert sums[0] == lanetest.chunk_sums_ref(want)[0], "chunk 0x%x" % c


def test_host_sweep_rejects_chunks_past_the_domain():
    lib = lanetest.load()
    sums = np.empty(2, np.uint64)
    assert lib.lanetest_ref_safe_denom(ctypes.c_uint32(lanetest.CHUNKS - 1), ctypes.c_uint32(2), ctypes.c_void_p(sums.ctypes.data), None) == -1
    assert lib.lanetest_ref_safe_denom(ctypes.c_uint32(lanetest.CHUNKS - 1), ctypes.c_uint32(1), ctypes.c_void_p(sums.ctypes.data), None) == 0


@pytest.mark.parametrize("fn", ["clampRound", "clampHigh"])
def test_sweep_table_holds_every_upper_clamp_the_sources_pass(fn):
    found = lanetest.find_clamp_sites(fn)
    assert found == set(lanetest.CLAMP_SITES[fn]), "call sites and tests/lanetest.py CLAMP_SITES differ: %s" % sorted(found ^ set(lanetest.CLAMP_SITES[fn]))
    passed = {v for vals in lanetest.CLAMP_SITES[fn].values() for v in vals}
    swept = {hi for name, (dev, hi, ref, args) in lanetest.SWEEPS32.items() if name.startswith("clampRound" if fn == "clampRound" else "cvt_pk_u8(clampHigh")}
    assert swept == passed | set(lanetest.CLAMP_EXTRA[fn])
    assert passed <= swept
