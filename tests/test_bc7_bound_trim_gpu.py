"""The straight-line first-tier partition bounds of the BC7 kernel (bc7_kernel.hip: subsetBound2D -- no early return for small
subsets, lam clamped at zero ahead of the square root, 1/n from the rounded-down table kRcpDown) and the last-round index clamp
of its fast dual-plane search (cvtt_kernel_common.h: clampHigh), block for block against the CPU oracle and pruned against
exhaustive.  A bound that came out too high, or an index byte that differs, shows as a block that differs.  The table itself
is checked on the CPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import content
from convectionkernels_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _api():
    from convectionkernels_amd import api
    return api


def _diff(a, b):
    return np.nonzero((np.asarray(a) != np.asarray(b)).any(axis=1))[0]


def _check(gpu_ctx, oracle_lib, blocks, opt, what):
    """pruned == oracle and pruned == exhaustive, block for block"""
    import torch
    api = _api()
    plan = api.BC7EncodingPlan()
    rcp = oracle_lib.probe_rcp()
    gpu_ctx.set_rcp_table(rcp)
    t = torch.from_numpy(blocks).cuda()
    exp = oracle_lib.encode_bc7(blocks, np.frombuffer(opt.tobytes(), np.uint8).copy(),
                                np.frombuffer(plan.tobytes(), np.uint8).copy(), rcp, threads=16)
    try:
        gpu_ctx.set_exhaustive(False)
        pruned = gpu_ctx.encode_bc7(t, opt, plan).cpu().numpy()
        gpu_ctx.set_exhaustive(True)
        full = gpu_ctx.encode_bc7(t, opt, plan).cpu().numpy()
    finally:
        gpu_ctx.set_exhaustive(False)
    bad = _diff(pruned, full)
    assert bad.size == 0, "%s: pruned != exhaustive at blocks %s" % (what, bad[:8])
    bad = _diff(pruned, exp)
    assert bad.size == 0, "%s: pruned != oracle at blocks %s" % (what, bad[:8])
    return pruned


def subset_edge_blocks(seed):
    """(256, 16, 4) uint8, four groups of 64 = one block per partition index.  The pixels of every subset of the block's own
    partition are either exactly collinear (base + k * step with integer steps: the scatter matrix has rank one, so the
    smaller eigenvalue the bound computes comes out slightly below zero) or of a single colour (a = b = c = 0).  Every block
    meets every partition of both tables in its bounds, i.e. every subset size they contain.
      0..63    two-subset shapes, alpha on the subset's line (RGBA bound set)
      64..127  two-subset shapes, alpha 255: waves without a translucent pixel (RGB sets, modes 1 / 3 ahead of mode 7)
      128..191 three-subset shapes, alpha 255
      192..255 waves that mix the two: even blocks three-subset shapes with alpha, odd blocks two-subset shapes, opaque"""
    from tools import gen_tables
    rng = np.random.Generator(np.random.PCG64(seed))
    px = np.arange(16)
    out = np.zeros((256, 16, 4), np.uint8)
    for i in range(256):
        group, part = divmod(i, 64)
        three = group == 2 or (group == 3 and i % 2 == 0)
        alpha = group == 0 or (group == 3 and i % 2 == 0)
        owner = ((gen_tables.P3[part] >> (2 * px)) & 3) if three else ((gen_tables.P2[part] >> px) & 1)
        blk = np.zeros((16, 4), np.int64)
        for s in range(3 if three else 2):
            members = np.nonzero(owner == s)[0]
            single = (part + s + group) % 3 == 0
            step = np.zeros(4, np.int64) if single else rng.integers(-7, 8, 4)
            k = rng.permutation(len(members))
            span = step * (len(members) - 1)
            lo = np.maximum(0, -span)
            hi = np.minimum(255, 255 - span)
            base = rng.integers(lo, hi + 1)
            blk[members] = base[None, :] + k[:, None] * step[None, :]
        if not alpha:
            blk[:, 3] = 255
        assert blk.min() >= 0 and blk.max() <= 255
        out[i] = blk
    return out


def test_subset_sizes_of_the_tables():
    """what `subset_edge_blocks` relies on: the partition tables hold subsets of 2..13 pixels, all inside the 17-entry table"""
    from tools import gen_tables
    px = np.arange(16)
    sizes = set()
    for part in range(64):
        n1 = bin(gen_tables.P2[part]).count("1")
        sizes |= {n1, 16 - n1}
        owner = (gen_tables.P3[part] >> (2 * px)) & 3
        sizes |= {int((owner == s).sum()) for s in range(3)}
    assert min(sizes) >= 1 and max(sizes) <= 15
    assert {2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13} <= sizes


def test_rcp_down_table():
    """kRcpDown[n] (cvtt_kernel_common.h): never above the exact 1/n and less than one ulp below it; entry 0 is 0"""
    src = open(os.path.join(ROOT, "convectionkernels_amd", "csrc", "cvtt_kernel_common.h")).read()
    m = re.search(r"kRcpDown\[17\]\s*=\s*\{([^}]*)\}", src)
    assert m, "kRcpDown not found"
    bits = np.array([int(x.strip().rstrip("u"), 16) for x in m.group(1).split(",")], np.uint32)
    assert bits.size == 17 and bits[0] == 0
    vals = bits.view(np.float32)
    for n in range(1, 17):
        v = vals[n]
        up = np.nextafter(v, np.float32(2.0))
        assert Fraction(float(v)) <= Fraction(1, n) < Fraction(float(up)), n
        # ... at least as safe as what it replaces: v_rcp_f32 (1 ulp either way) under the 0.9999 factor of the bound
        assert Fraction(float(v)) >= Fraction(1, n) * Fraction(9999, 10000), n


@pytest.mark.gpu
def test_collinear_and_single_colour_subsets(gpu_ctx, oracle_lib):
    api = _api()
    blocks = subset_edge_blocks(7)
    _check(gpu_ctx, oracle_lib, blocks, api.Options(), "subset edges")


FAMILY_OPTIONS = {
    "default": {},
    "uniform": {"flags": "uniform"},
    # negative, zero and very large weights: 0 * inf and inf - inf in the index projection of the last refine round
    "weights": {"redWeight": -1.0, "greenWeight": 0.0, "blueWeight": 100.0, "alphaWeight": 1.0},
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(FAMILY_OPTIONS))
def test_content_families(gpu_ctx, oracle_lib, name):
    api = _api()
    kw = dict(FAMILY_OPTIONS[name])
    if kw.get("flags") == "uniform":
        kw["flags"] = api.Flags.Default | api.Flags.Uniform
    fam = synth.content_families(128, seed=11)
    blocks = np.concatenate([fam[k] for k in sorted(fam)])
    assert blocks.shape[0] == 1024
    _check(gpu_ctx, oracle_lib, blocks, api.Options(**kw), name)


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", [1, 3])
def test_refine_rounds(gpu_ctx, oracle_lib, rounds):
    """one round: the first round is the last; three: two rounds feed the refiner ahead of it.  Dual-plane content (the
    winners are modes 4 and 5) and noise."""
    api = _api()
    blocks = np.concatenate([content.dual_plane_blocks(5, per=4), content.config_blocks(12, 32, 16)])
    assert blocks.shape[0] == 64
    _check(gpu_ctx, oracle_lib, blocks, api.Options(refineRoundsBC7=rounds), "refineRoundsBC7=%d" % rounds)
