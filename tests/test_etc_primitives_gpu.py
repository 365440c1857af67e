"""The small device functions of the ETC colour kernel (csrc/etc2_metric.h) swept on the device over their whole domains: the
fake-BT.709 resolvers, the three metrics one and two colours at a time, planarDecode and the T / H emitters
(tests/device/lanetest_etc.hip, tests/etc_parts.py, oracle/etc_parts.h).  The functions are the product header's own,
compiled with the product's flags into the lane-test library.  The expected values are the restatement's functions
(oracle/cvtt_oracle_etc_parts.inc) on the same input numbers -- tests/test_etc_primitives_cpu.py holds those equal to the
reference's own functions over the same domains -- and, for the emitters, the block decoded again by the product's decoder.
Every comparison is for equality; a failure names the function, the count of mismatches and the lowest mismatching input
with its arguments and both values."""
import ctypes

import numpy as np
import pytest

import etc_parts as P
import lanetest
from oracle import pyref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lt(gpu_ctx):
    return lanetest.load()


@pytest.mark.parametrize("name", list(P.SWEEPS))
def test_device_function_equals_the_restatement_on_its_whole_domain(lt, oracle_lib, name):
    msg = P.device_mismatches(name, oracle_lib)
    assert msg is None, msg
    if P.SWEEPS[name][0] in ("resolve_th", "resolve_half"):
        # the results are equal, so the device's stay inside the field where the host's do: 0 ... 15 (differential: 0 ... 31)
        assert P.host_sums(oracle_lib, name)[1] == 0, "%s: a channel leaves its field" % name


def test_sweep_reports_the_lowest_input_of_a_wrong_pairing(lt, oracle_lib):
    """the machinery itself: the individual table form held against the differential one must name the lowest input on which
    the two quantisers part, which the restatement finds on its own"""
    ind, dif = "resolveHalfFake (table form, individual)", "resolveHalfFake (table form, differential)"
    a, b = P.host_chunk(oracle_lib, ind, 0), P.host_chunk(oracle_lib, dif, 0)
    first = int(np.flatnonzero(a != b)[0])
    msg = P.device_mismatches(ind, oracle_lib, host_name=dif)
    want = "the lowest input %d (%s): the device gives 0x%x, the host 0x%x" % (first, P.describe(ind, first), a[first], b[first])
    assert msg is not None and want in msg, (msg, want)


def test_planar_decode_is_the_bit_replication(lt):
    got = P.device_chunk("planarDecode", 0)[:3 * 128].reshape(3, 128)
    c = np.arange(128, dtype=np.uint32)
    for ch in range(3):
        want = ((c << 1) | (c >> 6)) if ch == 1 else ((c << 2) | (c >> 4))
        n = 128 if ch == 1 else 64  # 7 bits of green, 6 of red and blue
        msg = lanetest.first_difference("planarDecode(coeff, %d)" % ch, got[ch][:n], want[:n], lambda i: "coeff %d" % i)
        assert msg is None, msg
        assert got[ch][:n].max() == 255 and got[ch][0] == 0


@pytest.mark.parametrize("fn", ["emitT", "emitH"])
def test_emitted_block_decodes_to_its_arguments(lt, fn):
    """every colour pair x table x opacity x four selector patterns: the block is T (H) mode by the format's overflow rule,
    carries the opaque bit, and the product's decoder gives, for texel p = 4 y + x,
      emitT: selector (packedSelectors >> 2 p) & 3 -> 17 isolated, 17 line + d, 17 line, 17 line - d, clamped, d = thDistance[table];
      emitH: sector bit p -> colour 0 or 1, sign bit p set -> - d, clear -> + d, d = thDistance of the whole 3-bit table, whichever
             order the emitter stores the colours in; equal colours decode as T mode to the same texels;
    without the opaque bit the format's index 2 is transparent black: in T mode that is selector 2, in H mode the texel whose
    stored sector bit is set and sign bit clear, read from the emitted word.  Equal H colours without opacity cannot avoid
    index 2 and are held to the reference's bytes only (the word sweeps)."""
    part = pyref.ETC_PARTS["emit_t" if fn == "emitT" else "emit_h"]
    count, lowest = lanetest.reduced("lanetest_etc_round_trip", ctypes.c_int(part), lanetest.ptr(P.device_tables()))
    n, pattern = lowest >> 2, lowest & 3
    assert count == 0, "%s: %d of 2^30 blocks decode to other texels, the lowest input %d (%s), pattern %d" % (
        fn, count, n, P.describe(fn + " high word", n), pattern)


@pytest.mark.parametrize("fn", ["emitT", "emitH"])
def test_in_kernel_decode_is_the_decode_entry_point(lt, gpu_ctx, fn):
    """the tables the sweeps read (filled from the product's table headers) against the ones the shim uploads: a sample of
    emitted blocks through Context.decode gives the texels the in-kernel decoder gave"""
    import torch
    rng = np.random.Generator(np.random.PCG64(20261024))
    inputs = rng.integers(0, 1 << 28, 4096, dtype=np.uint64).astype(np.uint32)
    opaque = ((inputs >> 27) & 1).astype(bool)
    d_in = lanetest.to_device(inputs.view(np.int32))
    blocks = torch.empty((len(inputs), 8), dtype=torch.uint8, device="cuda:0")
    texels = torch.empty((len(inputs), 16, 4), dtype=torch.uint8, device="cuda:0")
    part = pyref.ETC_PARTS["emit_t" if fn == "emitT" else "emit_h"]
    lanetest._check(lt.lanetest_etc_emit_sample(ctypes.c_int(part), lanetest.ptr(d_in), ctypes.c_uint32(len(inputs)), lanetest.ptr(P.device_tables()),
                                                lanetest.ptr(blocks), lanetest.ptr(texels), lanetest._stream()), "lanetest_etc_emit_sample")
    torch.cuda.synchronize()
    blocks, texels = blocks.cpu().numpy(), texels.cpu().numpy()
    for fmt, pick in (("etc2", opaque), ("etc2punchthrough", ~opaque)):
        idx = np.flatnonzero(pick)
        idx = idx[:len(idx) // 8 * 8]
        assert len(idx) >= 1024
        got = gpu_ctx.decode(fmt, blocks[idx])
        bad = np.flatnonzero((got != texels[idx]).any(axis=(1, 2)))
        assert len(bad) == 0, "%s as %s: %d of %d blocks decode differently, the lowest input %d (%s)" % (
            fn, fmt, len(bad), len(idx), inputs[idx[bad[0]]], P.describe(fn + " high word", int(inputs[idx[bad[0]]])))
