"""The refine round of the BC7 dual-plane search (bc7_dual.h: evalDual) after its trims: the lower index clamp with the
rounding first (cvtt_kernel_common.h: roundClampLow), the block's pixels read from LDS as LDS, and the index sets carried in
the layout the pixel loop produces (bc7_chain.h: dualIndexSlot) until packDualPlane sorts them to their pixels.  Block for
block: pruned = CPU oracle and pruned = exhaustive.  An index that lands at another pixel, a set that loses a bit on the way
through the quad argmin, the commit or the parked words, or a clamp that rounds differently shows as a block that differs.

The layout is only exercised by blocks whose winner is a dual-plane mode, and only shows where the indexes differ from pixel
to pixel, so ahead of the comparison the layout tests assert on the oracle's bytes alone that all twelve configurations
(mode 4 x 4 rotations x 2 index selectors, mode 5 x 4 rotations) win at least 16 blocks each and that at every one of the 16
pixel positions both index sets take at least two values.  The input that satisfies this was chosen with the oracle on the
CPU: uniform channel weights (with the default weights blue, rotation 3, hardly ever wins the wide index set) and a plan of
the dual-plane modes alone."""
import numpy as np
import pytest

import block_fields as F
import census_cases as C
import content
from convectionkernels_amd import api, synth

CONFIGURATIONS = [(4, r, s) for r in range(4) for s in range(2)] + [(5, r, -1) for r in range(4)]

# first bit and width of the two index sets in stream order (BC7 format; pixel 0 is stored one bit short)
INDEX_FIELDS = {4: ((50, 2), (81, 3)), 5: ((66, 2), (97, 2))}


def _diff(a, b):
    return np.nonzero((np.asarray(a) != np.asarray(b)).any(axis=1))[0]


def _raw(s):
    return np.frombuffer(s.tobytes(), np.uint8).copy()


def dual_plane_plan():
    """modes 4 and 5 only, four seed points for every rotation and index selector"""
    p = C.single_mode_plan(4)
    for r in range(4):
        p.mode4SP[r][0] = p.mode4SP[r][1] = p.mode5SP[r] = 4
    return p


def index_sets(packed):
    """(n, 2, 16) int64: both index sets of mode 4 / 5 blocks by pixel position, -1 for blocks of other modes"""
    mode = F.bc7_mode(packed)
    out = np.full((len(mode), 2, 16), -1, np.int64)
    for m, fields in INDEX_FIELDS.items():
        rows = np.nonzero(mode == m)[0]
        if not rows.size:
            continue
        for s, (base, width) in enumerate(fields):
            for px in range(16):
                start = base + width * px - (1 if px else 0)
                out[rows, s, px] = F.le_bits(packed[rows], start, width - (0 if px else 1))
    return out


def configurations(packed):
    return list(zip(F.bc7_mode(packed).tolist(), F.bc7_rotation(packed).tolist(), F.bc7_index_selector(packed).tolist()))


def assert_exercises_the_layout(packed, what):
    """the two conditions on the oracle's bytes"""
    cfg = configurations(packed)
    for want in CONFIGURATIONS:
        n = cfg.count(want)
        assert n >= 16, "%s: configuration %s wins %d blocks, fewer than 16" % (what, want, n)
    idx = index_sets(packed)
    dual = idx[idx[:, 0, 0] >= 0]
    for s in range(2):
        for px in range(16):
            assert np.unique(dual[:, s, px]).size >= 2, "%s: index set %d is constant at pixel %d" % (what, s, px)


def layout_blocks():
    b = np.concatenate([content.dual_plane_blocks(3, per=32), content.dual_plane_blocks(4, per=32)])
    assert b.shape == (512, 16, 4)
    return b


def layout_flags():
    return {"fast": api.Flags.Default | api.Flags.Uniform, "slow": api.Flags.Better | api.Flags.Uniform}


def noise_blocks():
    """1 024 blocks of RGBA noise: the first 16 384 pixels' worth of the headline's generator"""
    b = synth.tile_blocks(synth.image_rgba8(2, 128, 128))
    assert b.shape == (1024, 16, 4)
    return b


_oracle_cache = {}


def oracle_bytes(orc, key, blocks, opt, plan):
    """the oracle's bytes of a case, computed once per session"""
    if key not in _oracle_cache:
        _oracle_cache[key] = orc.encode_bc7(blocks, _raw(opt), _raw(plan), orc.probe_rcp(), threads=16)
        _oracle_cache[key].setflags(write=False)
    return _oracle_cache[key]


def check(gpu_ctx, exp, blocks, opt, plan, what, encode=None):
    """pruned == exhaustive and pruned == oracle, block for block; encode(): the call that returns the packed blocks as a
    numpy array (default: encode_bc7 of `blocks`)"""
    encode = encode or (lambda: gpu_ctx.encode_bc7(blocks, opt, plan))
    try:
        gpu_ctx.set_exhaustive(False)
        pruned = encode()
        gpu_ctx.set_exhaustive(True)
        full = encode()
    finally:
        gpu_ctx.set_exhaustive(False)
    bad = _diff(pruned, full)
    assert bad.size == 0, "%s: pruned != exhaustive at blocks %s" % (what, bad[:8])
    bad = _diff(pruned, exp)
    assert bad.size == 0, "%s: pruned != oracle at %d blocks, first %s: expected %s, got %s" % (
        what, bad.size, bad[:8], F.bc7_label(exp[bad[:1]])[0], F.bc7_label(pruned[bad[:1]])[0])


@pytest.mark.parametrize("indexing", ["fast", "slow"])
def test_layout_input_reaches_every_configuration_and_pixel(oracle_lib, indexing):
    """the conditions hold for the chosen input (CPU only: the GPU tests assert them again ahead of their comparison)"""
    opt = api.Options(flags=layout_flags()[indexing])
    exp = oracle_bytes(oracle_lib, ("layout", indexing), layout_blocks(), opt, dual_plane_plan())
    assert_exercises_the_layout(exp, indexing)


def test_index_sets_reader():
    """index_sets against a block written bit by bit: mode 5, index sets 0..3 cycling one way and the other"""
    bits = np.zeros(128, np.uint8)
    bits[5] = 1
    first = [p % 2 if p == 0 else p % 4 for p in range(16)]
    second = [(15 - p) % 4 if p else 1 for p in range(16)]
    for base, vals in ((66, first), (97, second)):
        for p, v in enumerate(vals):
            start = base + 2 * p - (1 if p else 0)
            for k in range(2 if p else 1):
                bits[start + k] = (v >> k) & 1
    packed = np.packbits(bits, bitorder="little")[None, :]
    got = index_sets(packed)
    assert got[0, 0].tolist() == first and got[0, 1].tolist() == second


@pytest.mark.gpu
@pytest.mark.parametrize("flags", ["default", "uniform", "better"])
@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_refine_rounds_on_noise(gpu_ctx, oracle_lib, rounds, flags):
    """one round: only a last round; two: one round that feeds the refiner; three: two of them"""
    f = {"default": api.Flags.Default, "uniform": api.Flags.Default | api.Flags.Uniform, "better": api.Flags.Better}[flags]
    opt, plan = api.Options(flags=f, refineRoundsBC7=rounds), api.BC7EncodingPlan()
    gpu_ctx.set_rcp_table(oracle_lib.probe_rcp())
    blocks = noise_blocks()
    exp = oracle_bytes(oracle_lib, ("noise", rounds, flags), blocks, opt, plan)
    check(gpu_ctx, exp, blocks, opt, plan, "noise, %s, refineRoundsBC7=%d" % (flags, rounds))


@pytest.mark.gpu
@pytest.mark.parametrize("indexing", ["fast", "slow"])
def test_every_configuration_and_pixel_position(gpu_ctx, oracle_lib, indexing):
    opt, plan = api.Options(flags=layout_flags()[indexing]), dual_plane_plan()
    gpu_ctx.set_rcp_table(oracle_lib.probe_rcp())
    blocks = layout_blocks()
    exp = oracle_bytes(oracle_lib, ("layout", indexing), blocks, opt, plan)
    assert_exercises_the_layout(exp, indexing)
    check(gpu_ctx, exp, blocks, opt, plan, "dual-plane content, %s indexing" % indexing)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 15, 16, 17, 1000])
def test_ragged_placements(gpu_ctx, oracle_lib, count):
    """`count` blocks as one block row of an image, the only way a caller hands over a number of blocks that is no multiple of
    eight: the row is tiled into groups of eight with clamped reads (half a wave, one wave, one and a half, and 62 and a half
    for 1 000), encoded, and compacted again.  Dual-plane content, its eight kinds interleaved so that the shortest row already
    holds more than one, default plan."""
    import torch
    opt, plan = api.Options(), api.BC7EncodingPlan()
    gpu_ctx.set_rcp_table(oracle_lib.probe_rcp())
    i = np.arange(count)
    blocks = content.dual_plane_blocks(9, per=125)[(i % 8) * 125 + i // 8]
    image = np.ascontiguousarray(blocks.reshape(count, 4, 4, 4).transpose(1, 0, 2, 3).reshape(4, 4 * count, 4))
    tiled = content.tile_clamped(image)
    assert (tiled[:count] == blocks).all() and tiled.shape[0] == (count + 7) // 8 * 8
    exp = content.compact_rows(oracle_bytes(oracle_lib, ("ragged", count), tiled, opt, plan), 4 * count, 4)
    assert exp.shape[0] == count
    t = torch.from_numpy(image).cuda()
    check(gpu_ctx, exp, None, opt, plan, "%d blocks" % count, lambda: gpu_ctx.encode_image("bc7", t, opt, plan).cpu().numpy())
