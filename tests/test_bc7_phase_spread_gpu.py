"""BC7 on RGBA noise at the sizes where the main launch's resident waves matter (tools/bc7_phase_overlap.py):
half a wave, one wave, and 65 536 + 24 blocks = 4 097 full waves and a part-filled one -- one wave more than the 4 096 that a
256-CU device holds at once, so a wave of the first resident generation and waves that refill a freed slot both run.  Whatever
order the resident waves issue in, the bytes are those of the exhaustive search and of the CPU oracle, and the same twice."""
import numpy as np
import pytest

from convectionkernels_amd import api, synth

SIZES = (8, 16, 65536 + 24)
EDGE = 256  # blocks compared with the oracle at either end (whole groups of eight: they encode alike on their own)


@pytest.fixture(scope="module")
def noise():
    blocks = synth.tile_blocks(synth.image_rgba8(26, 1024, 1024))  # 65 536 blocks
    return np.ascontiguousarray(np.concatenate([blocks, blocks[:24][:, ::-1]]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_noise_bytes(gpu_ctx, oracle_lib, noise, n):
    import torch
    assert len(noise) == SIZES[-1]
    rcp = oracle_lib.probe_rcp()
    gpu_ctx.set_rcp_table(rcp)
    opt, plan = api.Options(), api.BC7EncodingPlan()
    t = torch.from_numpy(noise[:n].copy()).cuda()
    try:
        gpu_ctx.set_exhaustive(False)
        a = gpu_ctx.encode_bc7(t, opt, plan).cpu().numpy()
        again = gpu_ctx.encode_bc7(t, opt, plan).cpu().numpy()
        gpu_ctx.set_exhaustive(True)
        full = gpu_ctx.encode_bc7(t, opt, plan).cpu().numpy()
    finally:
        gpu_ctx.set_exhaustive(False)
    assert a.shape[0] == n
    assert np.array_equal(a, again), "two encodes in a row differ"
    assert np.array_equal(a, full), "pruned != exhaustive at blocks %s" % np.flatnonzero((a != full).any(axis=1))[:8]
    o, p = np.frombuffer(opt.tobytes(), np.uint8).copy(), np.frombuffer(plan.tobytes(), np.uint8).copy()
    edge = min(EDGE, n)
    first = oracle_lib.encode_bc7(noise[:edge], o, p, rcp, threads=16)
    assert np.array_equal(a[:edge], first), "first blocks != oracle at %s" % np.flatnonzero((a[:edge] != first).any(axis=1))[:8]
    if n > edge:
        assert (n - edge) % 8 == 0
        last = oracle_lib.encode_bc7(np.ascontiguousarray(noise[n - edge:n]), o, p, rcp, threads=16)
        assert np.array_equal(a[n - edge:], last), "last blocks != oracle at %s" % (n - edge + np.flatnonzero((a[n - edge:] != last).any(axis=1))[:8])
