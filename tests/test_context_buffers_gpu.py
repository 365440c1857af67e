"""The buffers a context grows on demand (csrc/shim_internal.h, csrc/hip_owned.h): on ONE context each of them is used, made to
regrow, and used again with the first size -- the pipeline staging of the host entries, the measure buffers of cvttmi_measure_error,
the punch-through trial table of BC7 and the page-locked tables of the resize slots.  Then the context is closed and a second one
repeats the first leg.  Expected bytes never come from the GPU: the C oracle for the encodes, texture_decode_ref.py (and
tests/golden/decode.npz for BC6H) for the measures, resize_ref.py for the resizes.  The shapes are the smallest that take each path."""
import os

import numpy as np
import pytest

import content
import resize_ref
import texture_decode_ref as R
from convectionkernels_amd import api

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# 4104 x 64 B of PixelBlockU8 is just above the 256 KiB (2048 blocks x 128 B) the 8-blocks-per-call path reserves once
SMALL, LARGE = 8, 4104


def _bytes(s):
    return np.frombuffer(s.tobytes(), np.uint8).copy()


def _staging_leg(ctx, oracle_lib, rcp, blocks, want):
    """encode_bc7 from pageable numpy memory: 8 blocks, 4104 blocks (the staging regrows), 8 blocks again"""
    opt, plan = api.Options(), api.BC7EncodingPlan()
    for n in (SMALL, LARGE, SMALL):
        got = ctx.encode_bc7(blocks[:n].copy(), opt, plan)
        assert got.shape == (n, 16) and (got == want[:n]).all(), "encode_bc7 of %d blocks: %s" % (n, np.nonzero((got != want[:n]).any(axis=1))[0][:8])


def _measure_case(fmt):
    """8 packed blocks, their decoded form and a source to measure against"""
    rng = np.random.Generator(np.random.PCG64(2800 + R.FORMATS[fmt][0]))
    if fmt == "bc6hu":
        g = np.load(os.path.join(GOLD, "decode.npz"))
        packed, decoded = np.ascontiguousarray(g["bc6u_in"][:8]), np.ascontiguousarray(g["bc6u_out"][:8])
        source = rng.uniform(0.0, 4.0, (8, 16, 4)).astype(np.float16).view(np.int16)
    else:
        packed = rng.integers(0, 256, (8, R.FORMATS[fmt][1]), dtype=np.uint8)
        decoded = R.decode(fmt, packed)
        source = rng.integers(0, 256, (8, 16, 4), dtype=np.uint8)
    want, per_block = R.measure(fmt, decoded, source)
    return packed, source, want, per_block


def test_every_grown_buffer_is_used_regrown_and_used_again(oracle_lib):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    rcp = oracle_lib.probe_rcp()
    ctx = api.Context(0)
    ctx.set_rcp_table(rcp)

    # pipeline staging
    blocks = content.mixed_ldr_blocks(2801, LARGE // 8)
    want = oracle_lib.encode_bc7(blocks, _bytes(api.Options()), _bytes(api.BC7EncodingPlan()), rcp, threads=8)
    _staging_leg(ctx, oracle_lib, rcp, blocks, want)

    # dMeasureHost: 64 B sources, then the 128 B sources of BC6H (the buffer regrows), then 64 B again
    cases = {fmt: _measure_case(fmt) for fmt in ("bc1", "bc6hu")}
    for fmt in ("bc1", "bc6hu", "bc1"):
        packed, source, exp, per_block = cases[fmt]
        rep = ctx.measure_error(fmt, source, packed, per_block=True)
        assert rep.texels == exp["texels"] == 128, fmt
        assert [int(rep.totals.sse[c]) for c in range(4)] == [int(v) for v in exp["sse"]], fmt
        assert [float(rep.totals.sseHdr[c]) for c in range(4)] == [float(v) for v in exp["sse_hdr"]], fmt
        assert rep.per_block.dtype == per_block.dtype and (rep.per_block == per_block).all(), fmt

    # dPtTrial: more than 2 refine rounds under BC7_RespectPunchThrough keep the trial table in HBM, 2 KB per round and wave
    pt = content.mixed_ldr_blocks(2802, 2)
    plan = api.BC7EncodingPlan()
    for rounds in (3, 4, 3):
        opt = api.Options(flags=api.Flags.Default | api.Flags.BC7_RespectPunchThrough, refineRoundsBC7=rounds)
        exp = oracle_lib.encode_bc7(pt, _bytes(opt), _bytes(plan), rcp, threads=8)
        got = ctx.encode_bc7(pt, opt, plan)
        assert (got == exp).all(), "refineRoundsBC7 = %d: blocks %s" % (rounds, np.nonzero((got != exp).any(axis=1))[0])

    # resize tables: the four slots of the ring take the small tables, the next four calls regrow every slot, the next four meet
    # slots that are large enough, and the last call meets a slot that still holds its tables (copied again, not rebuilt)
    def resized(w, h, dw, dh, seed):
        img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
        tables = (api.resize_taps(w, dw, "lanczos3"), api.resize_taps(h, dh, "lanczos3"))
        return img, resize_ref.resize(img, dw, dh, "lanczos3", api.MIP_FILTER_BOX, "clamp", tables=tables)
    small = [resized(8 + 4 * i, 8, 4, 4, i) for i in range(4)]       # four different sizes: four slots
    large = [resized(64 + 4 * i, 64, 48, 48, 10 + i) for i in range(4)]
    for img, exp in small + large + small + small[:1]:
        h, w = img.shape[:2]
        got = ctx.resize(torch.from_numpy(img).cuda(), exp.shape[1], exp.shape[0], kernel="lanczos3")
        assert (got.cpu().numpy() == exp).all(), "%dx%d -> %dx%d" % (w, h, exp.shape[1], exp.shape[0])

    ctx.close()
    again = api.Context(0)
    again.set_rcp_table(rcp)
    _staging_leg(again, oracle_lib, rcp, blocks, want)
    again.close()
