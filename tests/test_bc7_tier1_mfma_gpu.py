"""BC7, the first-tier partition sums on the matrix cores (csrc/bc7_bounds.h, "by the matrix cores"): the encoder's bytes stay
those of the CPU oracle and of the exhaustive search, for part-filled waves and images of ragged rows, on content that sits on
the edges of the sums; and the first-tier bounds stay bit-equal to those of the build before the change.

tests/golden/bc7_tier1_parent_bounds.npz was taken once on an MI355X from the bound-dump build of commit 2ab43b7 ("Mip and
resize kernels: one header for the shared rule, same code"), the parent of the change, with bc7_tier1_inputs.run_dump: the
sums are integers and the formula is the same, so every bound, the error it was compared with and the verdict must be equal
-- which also catches a bound that became smaller, as the soundness test cannot."""
import os

import numpy as np
import pytest

import bc7_tier1_inputs as T1
from convectionkernels_amd import api

COUNTS = (8, 16, 24, 40)  # half a wave; one; one and a half; two and a half: the rows of the blocks that are not there must not leak


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def _diff(a, b):
    return np.flatnonzero((_bytes(a) != _bytes(b)).any(axis=1))


def _oracle_bc7(oracle_lib, blocks, rcp):
    return oracle_lib.encode_bc7(blocks, np.frombuffer(api.Options().tobytes(), np.uint8).copy(),
                                 np.frombuffer(api.BC7EncodingPlan().tobytes(), np.uint8).copy(), rcp, threads=16)


@pytest.fixture(scope="module")
def expected(oracle_lib):
    """name -> the oracle's bytes of the family's 40 blocks (computed once; a prefix of whole groups of eight encodes alike)"""
    rcp = oracle_lib.probe_rcp()
    return rcp, {name: _oracle_bc7(oracle_lib, blocks, rcp) for name, blocks in T1.families().items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(T1.families()))
def test_bytes_equal_oracle_and_exhaustive(gpu_ctx, expected, name):
    import torch
    rcp, exp = expected
    gpu_ctx.set_rcp_table(rcp)
    blocks = T1.families()[name]
    try:
        for n in COUNTS:
            t = torch.from_numpy(blocks[:n].copy()).cuda()
            gpu_ctx.set_exhaustive(False)
            a = gpu_ctx.encode_bc7(t, api.Options(), api.BC7EncodingPlan()).cpu().numpy()
            gpu_ctx.set_exhaustive(True)
            b = gpu_ctx.encode_bc7(t, api.Options(), api.BC7EncodingPlan()).cpu().numpy()
            bad = _diff(a, exp[name][:n])
            assert bad.size == 0, "%s, %d blocks: pruned != oracle at blocks %s" % (name, n, bad[:8])
            bad = _diff(a, b)
            assert bad.size == 0, "%s, %d blocks: pruned != exhaustive at blocks %s" % (name, n, bad[:8])
    finally:
        gpu_ctx.set_exhaustive(False)


@pytest.mark.gpu
@pytest.mark.parametrize("row_blocks", (1, 15, 17))
def test_images_of_ragged_rows(gpu_ctx, oracle_lib, row_blocks):
    """encode_image: rows of 1, 15 and 17 blocks, two block rows, the pixels of every family side by side"""
    import torch
    rcp = oracle_lib.probe_rcp()
    gpu_ctx.set_rcp_table(rcp)
    fam = T1.families()
    src = np.concatenate([fam[k][:8] for k in sorted(fam)])  # 40 blocks
    w, h = 4 * row_blocks, 8
    img = np.zeros((h, w, 4), np.uint8)
    for i in range(2 * row_blocks):
        by, bx = divmod(i, row_blocks)
        img[4 * by:4 * by + 4, 4 * bx:4 * bx + 4] = src[(7 * i + row_blocks) % len(src)].reshape(4, 4, 4)
    t = torch.from_numpy(img).cuda()
    try:
        gpu_ctx.set_exhaustive(False)
        a = gpu_ctx.encode_image("bc7", t).cpu().numpy()
        gpu_ctx.set_exhaustive(True)
        b = gpu_ctx.encode_image("bc7", t).cpu().numpy()
    finally:
        gpu_ctx.set_exhaustive(False)
    assert a.shape[0] == 2 * row_blocks
    tiled = gpu_ctx.tile_image(t)
    exp = torch.from_numpy(_oracle_bc7(oracle_lib, tiled.cpu().numpy(), rcp)).cuda()
    if w % 32:
        exp = gpu_ctx.compact_rows(exp, w, h)
    bad = _diff(a, exp.cpu().numpy())
    assert bad.size == 0, "pruned != oracle at blocks %s" % bad[:8]
    bad = _diff(a, b)
    assert bad.size == 0, "pruned != exhaustive at blocks %s" % bad[:8]


@pytest.mark.gpu
def test_first_tier_bounds_equal_the_parents(oracle_lib, tmp_path):
    assert os.path.exists(T1.PARENT_FIXTURE), T1.PARENT_FIXTURE
    gold = np.load(T1.PARENT_FIXTURE)
    assert np.array_equal(gold["blocks"], T1.fixture_blocks()), "the fixture was taken from other inputs"
    keys, vals = T1.tier1_records(T1.run_dump(str(tmp_path), oracle_lib.probe_rcp()))
    assert len(gold["keys"]) > 0
    # both two-subset sets, the three-subset set, and every partition of each are there
    assert set(np.unique(gold["keys"][:, 1])) == {0, 1, 2}
    assert keys.shape == gold["keys"].shape and np.array_equal(keys, gold["keys"]), "the first-tier records are not those of the parent"
    bad = np.flatnonzero((vals != gold["vals"]).any(axis=1))
    assert bad.size == 0, "%d of %d records differ; first (block, set, mode, partition) %s: bound, error, dropped %s, the parent's %s" % (
        bad.size, len(vals), keys[bad[0]], vals[bad[0]], gold["vals"][bad[0]])
