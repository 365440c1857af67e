"""What the ETC part sweeps (tests/test_etc_primitives_gpu.py) rest on, checked without a device: the restatement's parts
(oracle/cvtt_oracle_etc_parts.inc) equal the reference's own functions (oracle/ref_etc_parts.cpp, where oracle/_ref was built)
over the same whole domains; no resolver leaves its field; the Python bindings, the checksum scheme, the tables of inputs and
the failure report behave as the sweeps assume; the lane-test library exports the device side and the table of sweeps reaches
every function of csrc/etc2_metric.h."""
import os
import re
import subprocess

import numpy as np
import pytest

import etc_parts as P
import lanetest
from oracle import pyref

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
RESOLVERS = [n for n in P.SWEEPS if P.SWEEPS[n][0] in ("resolve_th", "resolve_half")]


@pytest.fixture(scope="module")
def ref_parts():
    """the reference's own functions (only where oracle/_ref was built)"""
    if not pyref.RefEtcParts.available():
        pytest.skip("oracle/_ref/libcvtt_ref_etcparts.so not present")
    return pyref.RefEtcParts()


# ---- restatement == reference, whole domains -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(P.SWEEPS))
def test_restatement_part_equals_the_reference_function(oracle_lib, ref_parts, name):
    want, want_flagged = P.host_sums(ref_parts, name)
    got, got_flagged = P.host_sums(oracle_lib, name)
    msg = P.chunk_mismatches(name, want, got, lambda c: P.host_chunk(ref_parts, name, c), lambda c: P.host_chunk(oracle_lib, name, c),
                             sides=("the restatement", "the reference"))
    assert msg is None, msg
    assert got_flagged == want_flagged


@pytest.mark.parametrize("name", RESOLVERS)
def test_no_resolver_leaves_its_field(oracle_lib, name):
    """cvtt_oracle_etc2.inc and etc2_kernel.hip say resolveTHFake `may push a channel to 16`.  Over every cell boundary, midpoint
    and seeded targets per channel, cubed, at every granularity, with the quantised value the callers derive, it does not:
    at 15 the low and the high corner of the channel coincide (min(unq + 17, 255) = 255), so the octant with the channel's
    bit set ties with its twin earlier in the loop and the strict `<` never takes it.  The half-block resolvers stay inside
    0 ... 15 / 0 ... 31 the same way (accurate form) or by their clamp (table form)."""
    assert P.host_sums(oracle_lib, name)[1] == 0


def test_reference_resolver_stays_in_its_field_too(ref_parts):
    for name in RESOLVERS:
        assert P.host_sums(ref_parts, name)[1] == 0, name


def test_range_flag_is_raised_by_a_value_outside(oracle_lib):
    """the flag the tests above count: variant bit 2 packs the differential form against the individual field (etc_parts.h),
    where the flag must be on exactly the results with a channel above 15"""
    part, _, _, table = P.sweep_args("resolveHalfFake (table form, differential)")
    _, full, flagged = oracle_lib.etc_parts(part, 5, None, table, first_chunk=0, num_chunks=8, full=True)
    above = ((full & 255) > 15) | (((full >> 8) & 255) > 15) | (((full >> 16) & 255) > 15)
    assert above.any() and not above.all() and np.array_equal(full >> 31 != 0, above) and flagged == above.sum()
    _, plain, none = oracle_lib.etc_parts(part, 1, None, table, first_chunk=0, num_chunks=8, full=True)
    assert none == 0 and np.array_equal(plain, full & 0x7fffffff)


# ---- bindings, checksums, domain ends --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["resolveTHFake", "resolveHalfFake (accurate, differential)", "EtcErr::wu weighted (goldens)", "emitH low word",
                                  "emitT high word, a channel at 16", "planarDecode"])
def test_bindings_agree_with_each_other(oracle_lib, name):
    part, variant, weights, table = P.sweep_args(name)
    last = pyref.etc_parts_chunks(part, variant) - 1
    for chunk in sorted({0, last // 3, last}):
        sums, full, _ = oracle_lib.etc_parts(part, variant, weights, table, first_chunk=chunk, num_chunks=1, full=True)
        assert sums[0] == lanetest.chunk_sums_ref(full)[0]  # the scheme of tests/device/lanetest_checksum.h
        inputs = chunk * P.CHUNK + np.array([0, 1, 7, 8, 2049, 4095], np.uint32)
        assert np.array_equal(oracle_lib.etc_parts_at(part, inputs, variant, weights, table), full[inputs - chunk * P.CHUNK])
    # threads and chunk ranges do not change a checksum
    n = min(last + 1, 24)
    a = oracle_lib.etc_parts(part, variant, weights, table, first_chunk=last + 1 - n, num_chunks=n, threads=5)[0]
    b = np.concatenate([oracle_lib.etc_parts(part, variant, weights, table, first_chunk=c, num_chunks=1)[0] for c in range(last + 1 - n, last + 1)])
    assert np.array_equal(a, b)


def test_reference_binding_takes_single_inputs(oracle_lib, ref_parts):
    for name in ("resolveTHFake", "EtcErr::operator() fake", "emitT low word"):
        part, variant, weights, table = P.sweep_args(name)
        rng = np.random.Generator(np.random.PCG64(5))
        inputs = rng.integers(0, pyref.etc_parts_chunks(part, variant) * P.CHUNK, 512, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(ref_parts.etc_parts_at(part, inputs, variant, weights, table), oracle_lib.etc_parts_at(part, inputs, variant, weights, table)), name


def test_host_sweeps_reject_what_lies_past_the_domain(oracle_lib):
    for part in pyref.ETC_PARTS:
        for variant in (0, 2):
            n = pyref.etc_parts_chunks(part, variant)
            table = np.zeros(16 * 128, np.int32)
            oracle_lib.etc_parts(part, variant, None, table, first_chunk=n - 1, num_chunks=1)
            with pytest.raises(ValueError):
                oracle_lib.etc_parts(part, variant, None, table, first_chunk=n - 1, num_chunks=2)
            with pytest.raises(ValueError):
                oracle_lib.etc_parts_at(part, np.array([n * P.CHUNK], np.uint32), variant, None, table)
    assert oracle_lib.lib.orc_etc_parts(len(pyref.ETC_PARTS), 0, None, None, 0, 0, None, None, None, 1) == -1


def test_t_emitter_on_a_hand_packed_block(ref_parts, oracle_lib):
    """hand-checked bytes: line colour (1, 2, 3), isolated (4, 9, 5), every selector value in every row, table 5, opaque --
    R overflows below zero (rh + rl = 1 < 4: bit 58 set, the three top bits clear), then rl, G, B, the line colour, table
    bits 2-1, the opaque bit, table bit 0; both emitters"""
    n = (1 << 27) | (5 << 24) | (4 << 12) | (9 << 16) | (5 << 20) | 1 | (2 << 4) | (3 << 8)
    hi = (1 << 26) | (1 << 27) | (0 << 24) | (9 << 20) | (5 << 16) | (1 << 12) | (2 << 8) | (3 << 4) | (2 << 2) | (1 << 1) | 1
    for lib in (oracle_lib, ref_parts):
        assert int(lib.etc_parts_at("emit_t", [n], 0)[0]) == hi


# ---- the tables of inputs --------------------------------------------------------------------------------------------------------
def test_th_table_holds_every_boundary():
    t = P.th_table()
    assert t.shape == (16, 128)
    for g in range(1, 17):
        row = set(t[g - 1].tolist())
        for k in range(16):
            assert {max(k * 34 * g - 1, 0), k * 34 * g, k * 34 * g + 1, k * 34 * g + 17 * g} <= row
        assert {510 * g, 638 * g} <= row and min(row) == 0 and max(row) == 638 * g
        assert len(row) == 128


def test_half_table_holds_every_step_of_every_quantiser():
    t = P.half_table()
    assert t.shape == (256,) and len(set(t.tolist())) == 256 and t.min() == 0 and t.max() == 2040
    have = set(t.tolist())
    cu = np.arange(2041)
    for q in P.half_quantisers(cu):
        steps = np.flatnonzero(np.diff(q)) + 1
        assert len(steps) >= 7
        for s in steps.tolist():
            assert {s - 1, s, min(s + 1, 2040)} <= have
    # an input takes 64 of the 256: four neighbouring (c0, c1) take them all (etc_parts.h, etcp_half_args)
    assert {i * 4 + ((c0 + 5) & 3) for i in range(64) for c0 in range(4)} == set(range(256))


def test_pixel_tables_hold_the_edges_and_an_exact_zero(oracle_lib):
    px = P.pixels()
    assert px.shape == (64, 3) and len({tuple(p) for p in px.tolist()}) == 64
    assert (0, 0, 0) in map(tuple, px.tolist()) and (255, 255, 255) in map(tuple, px.tolist())
    # every pixel meets its own colour: the uniform and the weighted metric then give exactly zero, whatever the weights
    own = ((px[:, 0].astype(np.uint32) << 16 | px[:, 1].astype(np.uint32) << 8 | px[:, 2].astype(np.uint32)) << 6) | np.arange(64, dtype=np.uint32)
    for name in ("EtcErr::wu uniform", "EtcErr::wu weighted (negative red)", "EtcErr::wu weighted (100, 1e-3, 0.1)", "EtcErr::operator() fake"):
        part, variant, weights, table = P.sweep_args(name)
        assert not oracle_lib.etc_parts_at(part, own, variant, weights, table).any(), name
    # and the fake-BT.709 pixels are the conversion the restatement makes: white's luma / chroma
    y, u, v = P.to_fake709(np.array([255, 255, 255]))
    assert abs(float(y) - 255 * 1.7320508) < 1e-3 and abs(float(u)) < 1e-3 and abs(float(v)) < 1e-3


# ---- the failure report ----------------------------------------------------------------------------------------------------------
def test_report_names_the_lowest_input_of_a_wrong_pairing(oracle_lib):
    """the individual table form against the differential one, chunks 0 ... 31: the message carries the count over the chunks
    that differ, the lowest input with its arguments, and both values"""
    ind, dif = "resolveHalfFake (table form, individual)", "resolveHalfFake (table form, differential)"
    pi, vi, _, table = P.sweep_args(ind)
    pd, vd, _, _ = P.sweep_args(dif)
    a_sums, a, _ = oracle_lib.etc_parts(pi, vi, None, table, 0, 32, full=True)
    b_sums, b, _ = oracle_lib.etc_parts(pd, vd, None, table, 0, 32, full=True)
    first = int(np.flatnonzero(a != b)[0])
    msg = P.chunk_mismatches(ind, b_sums, a_sums, lambda c: b[c * P.CHUNK:(c + 1) * P.CHUNK], lambda c: a[c * P.CHUNK:(c + 1) * P.CHUNK])
    assert msg.startswith("%s: %d of %d inputs differ, the lowest input %d (%s): the device gives 0x%x, the host 0x%x" % (
        ind, int((a != b).sum()), 32 * P.CHUNK, first, P.describe(ind, first), a[first], b[first])), msg
    assert "cumulative [" in msg
    assert P.chunk_mismatches(ind, a_sums, a_sums, None, None) is None


# ---- the device side ---------------------------------------------------------------------------------------------------------------
def test_lane_test_library_exports_the_device_side():
    assert os.path.exists(lanetest.LIB_PATH), "the default build makes libcvtt_lanetest.so (csrc/Makefile)"
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not installed")
    out = subprocess.check_output([READELF, "--dyn-syms", "--wide", lanetest.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " FUNC " in line and " GLOBAL " in line and " UND " not in line}
    assert not [s for s in P.DEVICE_SYMBOLS if s not in exported]
    from convectionkernels_amd import api
    product = api.load_library()
    for s in P.DEVICE_SYMBOLS:
        assert not hasattr(product, s), s


def test_sweep_table_reaches_every_function_of_the_header():
    """every function and struct of etc2_metric.h is swept or is called by a swept one, and the device file calls the header's
    own: it defines none of them and holds no copy of their constants"""
    header = lanetest._strip_comments(open(os.path.join(lanetest.CSRC, "etc2_metric.h")).read())
    defined = set(re.findall(r"__device__ __forceinline__ \w+ (\w+)\(", header)) | set(re.findall(r"^struct (\w+)", header, re.M))
    defined -= {"operator", "weigh2", "err2", "wu"}  # EtcErr's members
    assert defined == set(P.SWEPT_FUNCTIONS), defined ^ set(P.SWEPT_FUNCTIONS)
    device = lanetest._strip_comments(open(os.path.join(lanetest.ROOT, "tests", "device", "lanetest_etc.hip")).read())
    for call in ("resolveTHFake(", "resolveHalfFake(", "E(rec", "E.wu(", "E.weigh2(", "E.err2(", "planarDecode(", "emitT(", "emitH(", "etcColour<false>(", "etcColour<true>("):
        assert call in device, call
    for name in P.SWEPT_FUNCTIONS:
        assert not re.search(r"(void|int|float|struct)\s+%s\b\s*[({]" % name, device), name
    assert "0.368233989135369" not in device and '#include "etc2_metric.h"' in device
    swept = {P.SWEEPS[n][0] for n in P.SWEEPS}
    assert swept == set(pyref.ETC_PARTS)
    lane_makefile = open(os.path.join(lanetest.CSRC, "Makefile")).read()
    assert re.search(r"^LANEDEV :=.*\blanetest_etc\b", lane_makefile, re.M)
