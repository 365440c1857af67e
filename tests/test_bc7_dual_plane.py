"""The dual-plane search of BC7 modes 4 / 5 (evalDual, bc7_dual.h) on its own: plans that enable nothing else, so that every
block is decided by it, in each of the four kernel instantiations it is compiled into (fast / slow indexing x with / without
BC7_RespectPunchThrough), with 1..4 seed points, 1..3 refine rounds and uniform / default channel weights.

Content: the 128 directed dual-plane blocks of the mode census (tests/content.py dual_plane_blocks via census_cases: eight
waves, sixteen reference groups; one channel varies independently of the other three, wide / narrow either way).
CPU: the census -- under the default Options and four seed points the C restatement emits all twelve configurations
(mode 4 in every rotation with both index selectors, mode 5 in every rotation), so the comparison below reaches them all.
GPU: the kernel's bytes against the restatement's for every combination.

(A few blocks still come out as mode 7: the reference reads the plan's mode-7 masks into a dead variable and scans all 64
partitions whenever a group has alpha, BC67.cpp:1573-1660, so no plan switches that mode off for this content.)"""
import itertools
import os

import numpy as np
import pytest

import block_fields as F
import census_cases as C
from convectionkernels_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED_POINTS = (1, 2, 3, 4)
REFINE_ROUNDS = (1, 2, 3)
INDEXING = {"fast": api.Flags.Default, "slow": api.Flags.Better}


def blocks():
    b = C.bc7_sets()["4"][1]
    assert b.shape == (128, 16, 4)
    return b


def dual_plane_plan(seed_points):
    """modes 4 and 5 only, `seed_points` for every rotation and index selector"""
    p = C.single_mode_plan(4)
    for r in range(4):
        p.mode4SP[r][0] = p.mode4SP[r][1] = p.mode5SP[r] = seed_points
    return p


def options(indexing, punch_through, uniform, rounds):
    flags = INDEXING[indexing]
    if punch_through:
        flags |= api.Flags.BC7_RespectPunchThrough
    if uniform:
        flags |= api.Flags.Uniform
    return api.Options(flags=flags, refineRoundsBC7=rounds)


def restatement(orc, opt, plan, rcp):
    return orc.encode_bc7(blocks(), np.frombuffer(opt.tobytes(), np.uint8).copy(), np.frombuffer(plan.tobytes(), np.uint8).copy(), rcp, threads=8)


def configurations(packed):
    """{(mode, rotation, index selector)} of packed blocks; index selector -1 for mode 5"""
    return set(zip(F.bc7_mode(packed).tolist(), F.bc7_rotation(packed).tolist(), F.bc7_index_selector(packed).tolist()))


def test_content_reaches_all_twelve_configurations(oracle_lib):
    # under the census golden's RCPPS table, so the condition does not depend on the host
    rcp = np.load(os.path.join(ROOT, "tests", "golden", "mode_census.npz"))["rcp"]
    out = restatement(oracle_lib, api.Options(), dual_plane_plan(4), rcp)
    want = {(4, r, s) for r in range(4) for s in range(2)} | {(5, r, -1) for r in range(4)}
    assert want <= configurations(out), sorted(want - configurations(out))


@pytest.mark.gpu
@pytest.mark.parametrize("punch_through", [False, True], ids=["plain", "punchthrough"])
@pytest.mark.parametrize("indexing", list(INDEXING))
def test_gpu_dual_plane_equals_restatement(gpu_ctx, oracle_lib, indexing, punch_through):
    rcp = oracle_lib.probe_rcp()
    gpu_ctx.set_rcp_table(rcp)
    src = blocks()
    for uniform, rounds, sp in itertools.product((False, True), REFINE_ROUNDS, SEED_POINTS):
        opt, plan = options(indexing, punch_through, uniform, rounds), dual_plane_plan(sp)
        exp = restatement(oracle_lib, opt, plan, rcp)
        got = gpu_ctx.encode_bc7(src, opt, plan)
        bad = np.nonzero((got != exp).any(axis=1))[0]
        if bad.size:
            i = bad[:1]
            pytest.fail("%s indexing%s, %s weights, %d refine rounds, %d seed points: %d of %d blocks differ; block %d: expected %s, got %s"
                        % (indexing, " + punch-through" if punch_through else "", "uniform" if uniform else "default", rounds, sp,
                           bad.size, len(exp), i[0], F.bc7_label(exp[i])[0], F.bc7_label(got[i])[0]))
