"""Inputs and dump handling shared by tests/test_bc7_tier1_mfma_gpu.py (a helper, not a test): content that exercises the
first-tier partition sums of the BC7 kernel (csrc/bc7_bounds.h, "by the matrix cores"), and the first-tier records of a bound
dump (csrc/bc7_kernel.hip, CVTT_BC7_BOUND_DUMP) in an order that does not depend on which lane emitted them."""
import functools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DUMP_LIB = os.path.join(ROOT, "convectionkernels_amd", "lib", "variants", "libcvtt_mi355x_bounddump.so")
PARENT_FIXTURE = os.path.join(GOLD, "bc7_tier1_parent_bounds.npz")
FIXTURE_INPUTS = ("rgba_noise", "opaque_noise", "extremes")  # the three inputs of the fixture, 24 blocks each
FIXTURE_BLOCKS = 24


def _halves_and_checkerboards(n):
    """blocks whose pixels are (0, 0, 0, 0) or (255, 255, 255, 255): halves cut along every direction, both polarities, the
    1x1, 1x2, 2x1 and 2x2 checkerboards, then random half / half patterns.  Projections sit at +-127 there: uu = 16 129 and
    uv of both signs, the edges of the hi / lo split of the products."""
    y, x = np.divmod(np.arange(16), 4)
    pats = [x < 2, y < 2, x + y < 3, x > y, x + y <= 3, x >= y, (x + y) & 1, x & 1, y & 1, ((x >> 1) + (y >> 1)) & 1, (x >> 1) & 1, (y >> 1) & 1]
    pats = [np.asarray(p, bool) for p in pats]
    pats = pats + [~p for p in pats]
    rng = np.random.default_rng(250)
    while len(pats) < n:
        p = np.zeros(16, bool)
        p[rng.permutation(16)[:8]] = True
        pats.append(p)
    out = np.zeros((n, 16, 4), np.uint8)
    for i, p in enumerate(pats[:n]):
        out[i, p] = 255
    return out


def _two_colour_and_constant(n):
    rng = np.random.default_rng(251)
    out = np.zeros((n, 16, 4), np.uint8)
    for i in range(n):
        a, b = rng.integers(0, 256, (2, 4), dtype=np.uint8)
        if i % 3 == 1:
            a[3] = b[3] = 255
        if i % 4 == 3:
            b = a  # a constant block: every subset has zero variance
        out[i] = np.where((rng.integers(0, 2, 16) != 0)[:, None], a, b)
    return out


@functools.lru_cache(maxsize=None)
def families(n=40):
    """name -> (n, 16, 4) uint8 blocks"""
    rng = np.random.default_rng(252)
    noise = rng.integers(0, 256, (n, 16, 4), dtype=np.uint8)
    near = noise.copy()
    near[..., 3] = rng.integers(248, 256, (n, 16), dtype=np.uint8)  # partitions survive; blocks are handed over
    opaque = rng.integers(0, 256, (n, 16, 4), dtype=np.uint8)
    opaque[..., 3] = 255  # the RGB bound set serves mode 7 as well
    return {"rgba_noise": noise, "alpha_248_255": near, "opaque_noise": opaque, "two_colour": _two_colour_and_constant(n),
            "extremes": _halves_and_checkerboards(n)}


def tier1_records(records):
    """(keys (N, 4): block, bound set, mode, partition; values (N, 3): words 4, 6, 7 = the bound, the best error it was
    compared with, 1 = dropped) of every first-tier record that was formed (kinds 0 and 1), sorted by key"""
    r = np.asarray(records, np.uint32).reshape(-1, 12)
    r = r[((r[:, 1] & 0xff) == 2) & (((r[:, 1] >> 8) & 0xff) <= 1)]
    keys = np.stack([r[:, 0], r[:, 2] & 0xff, (r[:, 2] >> 8) & 0xff, r[:, 3] & 0xff], axis=1).astype(np.uint32)
    vals = r[:, [4, 6, 7]]
    both = np.concatenate([keys, vals], axis=1)
    order = np.lexsort(both.T[::-1])
    return keys[order], vals[order]


def fixture_blocks():
    """the fixture's inputs, 24 blocks each, as one array: blocks 0..23, 24..47, 48..71"""
    fam = families()
    return np.concatenate([fam[k][:FIXTURE_BLOCKS] for k in FIXTURE_INPUTS])


def run_dump(tmp, rcp, lib=DUMP_LIB):
    """tests/bc7_bound_dump_child.py with the dump build `lib` on fixture_blocks(), default Options: the records"""
    assert os.path.exists(lib), "%s is missing: `make -C convectionkernels_amd/csrc` builds it" % lib
    from convectionkernels_amd import api
    blocks = fixture_blocks()
    np.save(os.path.join(tmp, "blocks.npy"), blocks)
    cap = 1 << 18
    spec = {"blocks": os.path.join(tmp, "blocks.npy"), "rcp": [int(x) for x in np.asarray(rcp, np.float32).view(np.uint32)], "capacity": cap,
            "jobs": [{"name": "tier1", "n": int(blocks.shape[0]), "options": list(api.Options().tobytes()), "env": {}}]}
    with open(os.path.join(tmp, "jobs.json"), "w") as f:
        json.dump(spec, f)
    env = dict(os.environ, CVTTMI_LIB=lib)
    for k in ("CVTTMI_BC7_HARD_MIN", "CVTTMI_BC7_HARD_CAP", "CVTTMI_BC7_HARD_DIV"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bc7_bound_dump_child.py"), os.path.join(tmp, "jobs.json"),
                        os.path.join(tmp, "out.npz")], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, "the dump child ended with status %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    z = np.load(os.path.join(tmp, "out.npz"))
    assert int(z["count_tier1"][0]) <= cap, "the dump buffer overflowed"
    return z["records_tier1"]
