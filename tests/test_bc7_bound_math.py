"""The mathematics behind the sharper second-tier bound of the BC7 kernel (bc7_kernel.hip: subsetBoundSharp; DESIGN.md 4.1,
"Soundness of the bounds", part 3), restated in numpy and checked against encodings found by search: for random subsets of
smooth, photo-like and noisy blocks, NO pair of 8-bit end points with 2-bit or 3-bit BC7 interpolation (any mode's end points
are a subset of those) may reach an error below the bound -- neither with the subset's principal direction nor with a
perturbed one (the bound must hold for any unit vector).  CPU only; the kernel's own arithmetic is covered by the bit-exact
parity tests on the GPU (a bound that is too high there shows up as a block that differs from the reference)."""
import numpy as np

from bc7_bound_ref import W_DEFAULT as W  # default channel weights
from bc7_bound_ref import kmeans_1d, sharp_bound  # (shared with tests/test_bc7_bound_soundness.py, which holds the kernel's values to it)
from convectionkernels_amd import synth

WEIGHTS = {4: [0, 21, 43, 64], 8: [0, 9, 18, 27, 37, 46, 55, 64]}
PARTITIONS2 = [0xcccc, 0x8888, 0xeeee, 0xecc8, 0xc880, 0xfeec, 0xfec8, 0xec80, 0xc800, 0xffec, 0xfe80, 0xe800, 0xffe8, 0xff00, 0xfff0, 0xf000,
               0xf710, 0x008e, 0x7100, 0x08ce, 0x008c, 0x7310, 0x3100, 0x8cce, 0x088c, 0x3110, 0x6666, 0x366c, 0x17e8, 0x0ff0, 0x718e, 0x399c]


def error_of(q, e0, e1, levels):
    wt = np.array(WEIGHTS[levels])
    rec = ((e0[None, :] * (64 - wt[:, None]) + e1[None, :] * wt[:, None] + 32) >> 6).astype(np.float64)
    return ((((q[:, None, :] - rec[None, :, :]) * W) ** 2).sum(-1)).min(1).sum()


def search_encoding(q, levels):
    """a good (not necessarily optimal) encoding of the subset: PCA end points, then coordinate descent on the integers"""
    p = q * W
    c = p - p.mean(0)
    d = np.linalg.eigh(c.T @ c)[1][:, -1]
    t = c @ d
    best = None
    for sc in (1.0, 0.85, 1.1):
        e0 = np.clip(np.rint(q.mean(0) + (d / W) * t.min() * sc), 0, 255).astype(np.int64)
        e1 = np.clip(np.rint(q.mean(0) + (d / W) * t.max() * sc), 0, 255).astype(np.int64)
        cur = error_of(q, e0, e1, levels)
        improved = True
        while improved:
            improved = False
            for which in (0, 1):
                for ch in range(3):
                    for dv in (-2, -1, 1, 2):
                        f0, f1 = e0.copy(), e1.copy()
                        tgt = f0 if which == 0 else f1
                        tgt[ch] = np.clip(tgt[ch] + dv, 0, 255)
                        e = error_of(q, f0, f1, levels)
                        if e < cur:
                            cur, e0, e1, improved = e, f0, f1, True
        best = cur if best is None else min(best, cur)
    return best


def test_sharp_bound_never_exceeds_a_found_encoding():
    rng = np.random.default_rng(11)
    fam = synth.content_families(512)
    worst = 0.0
    for name in ("photo-like", "gradient opaque", "opaque noise"):
        for _ in range(40):
            blk = fam[name][rng.integers(512)][:, :3].astype(np.int64)
            part = PARTITIONS2[rng.integers(len(PARTITIONS2))]
            member = np.array([((part >> k) & 1) == rng.integers(2) for k in range(16)])
            q = blk[member]
            if len(q) < 3:
                continue
            levels = 4 if rng.integers(2) else 8
            p = q * W
            c = p - p.mean(0)
            d = np.linalg.eigh(c.T @ c)[1][:, -1]
            d2 = d + rng.normal(0, 0.05, 3)
            d2 /= np.linalg.norm(d2)
            found = search_encoding(q, levels)
            for dd in (d, d2):
                bound = sharp_bound(p, dd, levels)
                assert bound <= found + 1e-9, (name, levels, len(q), bound, found)
                worst = max(worst, bound / max(found, 1e-9))
    assert worst > 0.5  # ... and it is not vacuous: somewhere it comes within a factor of two of what the search found


def test_clustering_cost_is_exact_on_small_cases():
    rng = np.random.default_rng(3)
    for _ in range(30):
        t = rng.integers(0, 40, rng.integers(5, 9)).astype(np.float64)
        n = len(t)
        best = None
        # brute force over all assignments of the sorted values to 4 runs
        ts = np.sort(t)
        for a in range(1, n):
            for b in range(a, n):
                for c in range(b, n):
                    cost = sum(((g - g.mean()) ** 2).sum() for g in (ts[:a], ts[a:b], ts[b:c], ts[c:]) if len(g))
                    best = cost if best is None else min(best, cost)
        assert abs(kmeans_1d(t, 4) - best) < 1e-9
