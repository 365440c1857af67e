"""References for the pruning bounds of the BC7 kernel (test helper; tests/test_bc7_bound_soundness.py and
tests/test_bc7_bound_math.py).  Plain numpy float64, nothing of the kernel's float arithmetic:

  reference A   what the derivation claims (docs/history.md "Soundness of the bounds"): for a subset under the
                channel weights, R = trace(S) - lambda_max(S) of the weighted scatter matrix, delta = 0.5 sqrt(sum w^2), and
                g(R) = max(0, R - 2 delta sqrt(n R)) for R >= n delta^2, else 0; a partition's bound is the sum over its subsets, plus
                the static alpha error of the RGB modes (reference BC67.cpp:1250-1264).  `sharp_bound` is subsetBoundSharp
                without its float margins, for any unit vector d.
  reference B   what the reference encoder reaches: a BC7EncodingPlan that leaves one candidate (mode, partition | rotation
                and index selector), encoded by the C restatement, decoded here (`decode_bc7`, held to the reference decoder's
                recorded output in tests/golden/decode.npz) and measured against the source in the metric of the commit test.

Also the layout of the records of the kernel's bound dump (bc7_kernel.hip, CVTT_BC7_BOUND_DUMP)."""
import numpy as np

from convectionkernels_amd import api
from tools import gen_tables

TIERS = ("whole-6", "rot", "tier1", "full", "sharp", "probe-full", "probe-sharp")
T_WHOLE6, T_ROT, T_TIER1, T_FULL, T_SHARP, T_PROBE_FULL, T_PROBE_SHARP, T_FINAL = range(8)
K_FORM, K_FORM_CMP, K_RELOAD, K_SUBSET, K_END = range(5)
RECORD_WORDS = 12
RECORD_DTYPE = np.dtype([("block", "<u4"), ("tier", "u1"), ("kind", "u1"), ("hard", "u1"), ("pad0", "u1"),
                         ("set", "u1"), ("mode", "u1"), ("subsets", "u1"), ("bits", "u1"),
                         ("part", "u1"), ("sub", "u1"), ("pad1", "<u2"),
                         ("computed", "<f4"), ("stored", "<f4"), ("err", "<f4"), ("dropped", "<u4"), ("x", "<f4", (4,))])
assert RECORD_DTYPE.itemsize == 4 * RECORD_WORDS

# channel triples of the rotation bounds: rotation r codes channel r - 1 (alpha for r = 0) on its own
ROT_CHANNELS = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))
MODE_SUBSETS = {0: 3, 1: 2, 2: 3, 3: 2, 6: 1, 7: 2}
MODE_INDEX_BITS = {0: 3, 1: 3, 2: 2, 3: 2, 6: 4, 7: 2}
# bound set -> the modes a value of the set may be held to, by the index bits it was computed for (4 = any)
SET_MODES = {0: {4: (7,), 2: (7,), 3: ()}, 1: {4: (1, 3), 2: (3,), 3: (1,)}, 2: {4: (0, 2), 2: (2,), 3: (0,)}, 3: {4: (6,)}}

W_DEFAULT = np.array([np.float32(0.2125) / np.float32(0.7154), 1.0, np.float32(0.0721) / np.float32(0.7154)], np.float64)
BETAS = [0, 0.01, 0.02, 0.03, 0.04, 0.055, 0.07, 0.085, 0.1, 0.125, 0.15, 0.175, 0.2, 0.25, 0.3, 0.375, 0.45, 0.55, 0.7, 0.85, 1.0]
U24 = 2.0 ** -24


def weights(opt):
    """(w, wSq) as the shim hands them to the kernel: float32 values, here as float64; all ones under Flags::Uniform"""
    if opt.flags & api.Flags.Uniform:
        w = np.ones(4, np.float32)
    else:
        w = np.array([opt.redWeight, opt.greenWeight, opt.blueWeight, opt.alphaWeight], np.float32)
    return w.astype(np.float64), (w * w).astype(np.float64)


def subset_masks(subsets, partition):
    """pixel bitmaps of the subsets of a partition, subset 0 first"""
    if subsets == 1:
        return [0xFFFF]
    if subsets == 2:
        m1 = gen_tables.P2[partition]
        return [~m1 & 0xFFFF, m1]
    return gen_tables.subset_masks3(gen_tables.P3[partition])


def mask_matrix(masks):
    return np.array([[(m >> p) & 1 for p in range(16)] for m in masks], np.float64)


# ---------------------------------------------------------------- reference A
def slack(x, s, n):
    """error >= x - 2 s sqrt(n x) when every reconstructed colour is within s of the trial's line (clamped, monotone in x)"""
    return x - 2 * s * np.sqrt(n * x) if x > 4 * n * s * s else 0.0


def residuals(points_w, member):
    """R = trace(S) - lambda_max(S) of the weighted scatter matrix of every (block, subset): points_w (B, 16, C) weighted
    pixels, member (K, 16) 0 / 1 -> (R (B, K), n (K,))"""
    n = member.sum(1)
    nn = np.maximum(n, 1.0)
    mean = np.einsum("kp,bpc->bkc", member, points_w) / nn[None, :, None]
    S = np.einsum("kp,bpc,bpd->bkcd", member, points_w, points_w) - nn[None, :, None, None] * mean[..., :, None] * mean[..., None, :]
    lam = np.linalg.eigvalsh(S)[..., -1]
    R = np.trace(S, axis1=-2, axis2=-1) - lam
    return np.maximum(R, 0.0), n


def g_of(R, n, delta):
    """g(R) = R - 2 delta sqrt(n R) for R >= n delta^2, else 0 (no margin) -- and never below 0: between n delta^2 and
    4 n delta^2 the expression is negative, where the bound an error sum has anyway, zero, is the better one"""
    return np.where((R >= n * delta * delta) & (n >= 2), np.maximum(R - 2.0 * delta * np.sqrt(n * R), 0.0), 0.0)


def exact_subset_bound(points_w, delta):
    """g(R) of one subset: points_w (n, C) weighted pixels"""
    R, n = residuals(points_w[None], np.ones((1, len(points_w))))
    return float(g_of(R, n, delta)[0, 0])


def static_alpha(blocks, opt):
    """the static alpha error the reference adds in the RGB modes (BC67.cpp:1250-1264): sum (255 - a)^2, times the squared
    alpha weight unless Flags::Uniform; exact"""
    d = 255.0 - blocks[:, :, 3].astype(np.float64)
    return (d * d).sum(1) * weights(opt)[1][3]


class ExactBounds:
    """reference A for every (block, bound set | rotation, partition) of `blocks` under `opt`, computed when first asked"""

    def __init__(self, blocks, opt):
        self.blocks = np.asarray(blocks)
        self.opt = opt
        self.w, self.wsq = weights(opt)
        self.static = static_alpha(self.blocks, opt)
        self._cache = {}

    def delta(self, channels):
        return 0.5 * np.sqrt(sum(self.wsq[c] for c in channels))

    def subsets(self, channels, subsets):
        """g of every subset of every partition: (B, partitions, subsets)"""
        key = (tuple(channels), subsets)
        if key not in self._cache:
            parts = 1 if subsets == 1 else 64
            masks = [m for p in range(parts) for m in subset_masks(subsets, p)]
            pw = self.blocks[:, :, list(channels)].astype(np.float64) * self.w[list(channels)]
            R, n = residuals(pw, mask_matrix(masks))
            self._cache[key] = g_of(R, n[None, :], self.delta(channels)).reshape(len(self.blocks), parts, subsets)
        return self._cache[key]

    def set_bound(self, bound_set):
        """(B, partitions): sum over the subsets, plus the static alpha error for the RGB sets"""
        if bound_set == 0:
            return self.subsets((0, 1, 2, 3), 2).sum(2)
        if bound_set == 3:
            return self.subsets((0, 1, 2, 3), 1).sum(2)
        return self.subsets((0, 1, 2), 2 if bound_set == 1 else 3).sum(2) + self.static[:, None]

    def rotation_bound(self):
        """(B, 4): the three channels that share a line; the channel coded on its own costs >= 0"""
        return np.stack([self.subsets(ROT_CHANNELS[r], 1)[:, 0, 0] for r in range(4)], 1)


def kmeans_1d(t, k):
    """exact cost of the best clustering of t into k groups (the kernel's dynamic programme)"""
    t = np.sort(t)
    n = len(t)
    if n <= k:
        return 0.0
    p1 = np.concatenate([[0.0], np.cumsum(t)])
    p2 = np.concatenate([[0.0], np.cumsum(t * t)])
    i, j = np.triu_indices(n + 1, 1)
    cost = np.full((n + 1, n + 1), np.inf)  # cost[i, j]: one group of t[i .. j-1]
    cost[i, j] = (p2[j] - p2[i]) - (p1[j] - p1[i]) ** 2 / (j - i)
    d = cost[0].copy()
    d[0] = 0.0
    for _ in range(k - 1):
        d = np.minimum(d, (d[:, None] + cost).min(0))
    return max(d[n], 0.0)


_B0, _B1 = np.array(BETAS[:-1]), np.array(BETAS[1:])
_A1 = np.sqrt(1 - _B1 * _B1)
# the largest alpha * beta of an interval
_CROSS = np.where((_B0 <= np.sqrt(0.5)) & (np.sqrt(0.5) <= _B1), 0.5, np.maximum(_B0 * np.sqrt(1 - _B0 * _B0), _B1 * _A1))


def sharp_bound(points_w, d, levels, w=W_DEFAULT):
    """subsetBoundSharp without its float margins: points_w = weighted pixels (n, C), d = any unit vector, w = the C channel
    weights.  (The intervals of beta as arrays: every term at its worst value on the interval, the minimum over them.)"""
    w = np.abs(np.asarray(w, np.float64))
    w2 = float((w ** 2).sum())
    n = len(points_w)
    c = points_w - points_w.mean(0)
    S = c.T @ c
    T = np.trace(S)
    r_true = T - np.linalg.eigvalsh(S)[-1]
    L = d @ S @ d
    Rd = T - L
    rho = np.linalg.norm(S @ d - L * d)
    a = np.abs(d) * w
    md = max(0.0, 2 * a.max() - a.sum())
    perp = np.sqrt(max(w2 - md * md, 0.0))
    sq = np.sqrt(kmeans_1d(c @ d, levels)) if levels == 4 else 0.0  # the kernel computes Q_d for the two-bit modes only
    base = np.minimum((1 - _B0 * _B0) * Rd + _B0 * _B0 * L, (1 - _B1 * _B1) * Rd + _B1 * _B1 * L) - 2 * _CROSS * rho
    base = np.maximum(base, r_true)
    g = base + np.maximum(0.0, _A1 * sq - _B1 * np.sqrt(max(Rd, 0.0))) ** 2
    inner = np.maximum(0.0, _A1 * md - _B1 * perp)
    s = 0.5 * np.sqrt(np.maximum(w2 - inner * inner, 0.0))
    v = np.where(g > 4 * n * s * s, g - 2 * s * np.sqrt(n * np.maximum(g, 0.0)), 0.0)  # slack(g, s, n) per interval
    return max(slack(r_true, 0.5 * np.sqrt(w2), n), float(v.min()))


def lb_store(v):
    """what the kernel's bound table gives back for v >= 0: the upper 16 bits of the binary32 value (lbStore / lbLoad)"""
    bits = np.asarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)
    return np.abs(bits.view(np.float32))


# ---------------------------------------------------------------- reference B
def _fields(packed):
    bits = np.unpackbits(np.ascontiguousarray(packed, np.uint8).reshape(-1, 16), axis=1, bitorder="little").astype(np.int64)

    def take(start, count):
        return (bits[:, start:start + count] << np.arange(count, dtype=np.int64)).sum(1) if count else np.zeros(len(bits), np.int64)
    return take


# mode -> (subsets, partition bits, rotation bits, index-selector bits, colour bits, alpha bits, p-bits per subset: 0 none /
#          1 shared / 2 one per end point, index bits, secondary index bits)
_BC7 = {0: (3, 4, 0, 0, 4, 0, 2, 3, 0), 1: (2, 6, 0, 0, 6, 0, 1, 3, 0), 2: (3, 6, 0, 0, 5, 0, 0, 2, 0), 3: (2, 6, 0, 0, 7, 0, 2, 2, 0),
        4: (1, 0, 2, 1, 5, 6, 0, 2, 3), 5: (1, 0, 2, 0, 7, 8, 0, 2, 2), 6: (1, 0, 0, 0, 7, 7, 2, 4, 0), 7: (2, 6, 0, 0, 5, 5, 2, 2, 0)}


def _decode_group(packed, mode, partition):
    """blocks of one mode and one partition -> (n, 16, 4) int64"""
    ns, pbits, rbits, sbits, cb, ab, pmode, ib, ib2 = _BC7[mode]
    take = _fields(packed)
    n = len(packed)
    pos = mode + 1 + pbits
    rot = take(pos, rbits)
    pos += rbits
    sel = take(pos, sbits)
    pos += sbits
    ne = 2 * ns
    ep = np.zeros((n, ne, 4), np.int64)
    for ch in range(3):
        for e in range(ne):
            ep[:, e, ch] = take(pos, cb)
            pos += cb
    for e in range(ne):
        ep[:, e, 3] = take(pos, ab)
        pos += ab
    cbits, abits = cb, ab
    if pmode:
        for e in range(ne):
            p = take(pos + (e if pmode == 2 else e // 2), 1)
            ep[:, e, :3] = ep[:, e, :3] * 2 + p[:, None]
            if ab:
                ep[:, e, 3] = ep[:, e, 3] * 2 + p
        pos += ne if pmode == 2 else ns
        cbits += 1
        abits += 1 if ab else 0
    ep[:, :, :3] = (ep[:, :, :3] << (8 - cbits)) | (ep[:, :, :3] >> (2 * cbits - 8))
    if ab:
        ep[:, :, 3] = (ep[:, :, 3] << (8 - abits)) | (ep[:, :, 3] >> (2 * abits - 8))
    else:
        ep[:, :, 3] = 255
    masks = subset_masks(ns, partition)
    owner = np.array([[s for s in range(ns) if (masks[s] >> p) & 1][0] for p in range(16)])
    anchors = {0}
    if ns == 2:
        anchors.add(gen_tables.ANCHOR2[partition])
    elif ns == 3:
        anchors |= set(gen_tables.ANCHOR3[partition])

    def indexes(bits, anchor_set):
        nonlocal pos
        out = np.zeros((n, 16), np.int64)
        for p in range(16):
            k = bits - (1 if p in anchor_set else 0)
            out[:, p] = take(pos, k)
            pos += k
        return out
    idx = indexes(ib, anchors)
    idx2 = indexes(ib2, {0}) if ib2 else None
    assert pos == 128, (mode, pos)
    out = np.zeros((n, 16, 4), np.int64)
    rows = np.arange(n)
    for p in range(16):
        e0, e1 = ep[:, 2 * owner[p]], ep[:, 2 * owner[p] + 1]
        wc = np.array(gen_tables.WEIGHTS[ib])[idx[:, p]]
        if ib2:
            w2 = np.array(gen_tables.WEIGHTS[ib2])[idx2[:, p]]
            swap = sel == 1  # index selector 1: the secondary (wider) set interpolates the colours
            wcol = np.where(swap, w2, wc)
            walpha = np.where(swap, wc, w2)
        else:
            wcol = walpha = wc
        out[rows, p, :3] = (e0[:, :3] * (64 - wcol[:, None]) + e1[:, :3] * wcol[:, None] + 32) >> 6
        out[rows, p, 3] = (e0[:, 3] * (64 - walpha) + e1[:, 3] * walpha + 32) >> 6
    for r in (1, 2, 3):
        m = rot == r
        if m.any():
            t = out[m, :, 3].copy()
            out[m, :, 3] = out[m, :, r - 1]
            out[m, :, r - 1] = t
    return out


def decode_bc7(packed):
    """BC7 blocks (n, 16) uint8 -> (n, 16, 4) uint8; a block with the reserved mode byte 0 decodes to zeros"""
    import block_fields as F
    packed = np.ascontiguousarray(packed, np.uint8).reshape(-1, 16)
    mode, part = F.bc7_mode(packed), F.bc7_partition(packed)
    out = np.zeros((len(packed), 16, 4), np.uint8)
    for m in range(8):
        for p in np.unique(part[mode == m]):
            sel = np.nonzero((mode == m) & (part == p))[0]
            out[sel] = _decode_group(packed[sel], m, max(int(p), 0)).astype(np.uint8)
    return out


def block_error(blocks, decoded, opt):
    """weighted squared error per block in float64, in the metric of the reference's commit test: the squared differences of
    a channel summed, times the squared channel weight (all ones under Flags::Uniform)"""
    d = decoded.astype(np.int64) - np.asarray(blocks).astype(np.int64)
    return ((d * d).sum(1).astype(np.float64) * weights(opt)[1]).sum(1)


def candidates():
    """every candidate of the search: (mode, partition) for modes 0-3 and 7, (6, 0), (4, 2 * rotation + index selector),
    (5, rotation)"""
    out = [(0, p) for p in range(16)]
    for m in (1, 2, 3, 7):
        out += [(m, p) for p in range(64)]
    out += [(6, 0)] + [(4, k) for k in range(8)] + [(5, r) for r in range(4)]
    return out


_SHAPES = None


def single_candidate_plan(mode, which):
    """A BC7EncodingPlan that leaves one candidate, with the seed-point counts the default plan gives its shapes.  Modes 0-3:
    one bit of the mode's partition mask; modes 4 / 5: one rotation (and index selector); mode 6 alone.  The reference never
    reads the mode-7 partition masks where a group has alpha (BC67.cpp:1592-1597), so mode 7 is steered by the seed counts: a
    shape without seed points keeps its reset error FLT_MAX (BC67.cpp:1228-1242) and a partition with such a subset is never
    committed -- the RGBA counts are zero except for the two shapes of the wanted partition (the whole block for mode 6).  So
    every block of any group emits the candidate, except that modes 0-3 need a group that allows them (rgb_modes_allowed)."""
    global _SHAPES
    if _SHAPES is None:
        _SHAPES = gen_tables.derive()
    p = api.BC7EncodingPlan()
    default_rgba = list(p.seedPointsForShapeRGBA)
    p.mode0PartitionEnabled = 0
    p.mode1PartitionEnabled = p.mode2PartitionEnabled = p.mode3PartitionEnabled = 0
    p.mode6Enabled = 0
    for r in range(4):
        p.mode4SP[r][0] = p.mode4SP[r][1] = p.mode5SP[r] = 0
    for i in range(129):
        p.seedPointsForShapeRGBA[i] = 0
    if mode == 0:
        p.mode0PartitionEnabled = 1 << which
    elif mode == 1:
        p.mode1PartitionEnabled = 1 << which
    elif mode == 2:
        p.mode2PartitionEnabled = 1 << which
    elif mode == 3:
        p.mode3PartitionEnabled = 1 << which
    elif mode == 4:
        p.mode4SP[which >> 1][which & 1] = 4
    elif mode == 5:
        p.mode5SP[which] = 4
    elif mode == 6:
        p.mode6Enabled = 1
        p.seedPointsForShapeRGBA[0] = default_rgba[0]
    elif mode == 7:
        for s in _SHAPES["shapes2"][which]:
            p.seedPointsForShapeRGBA[s] = default_rgba[s]
    else:
        raise ValueError(mode)
    # The shape lists only say for which shapes the seeds are computed ahead of the search; a shape nothing searches (no seed
    # points, or its partitions off) may go from them.  Most of the time of a single-candidate encode is those seeds.
    needed = {0: _SHAPES["shapes3"], 2: _SHAPES["shapes3"], 1: _SHAPES["shapes2"], 3: _SHAPES["shapes2"],
              7: _SHAPES["shapes2"]}.get(mode)
    needed = sorted(needed[which]) if needed is not None else [0]
    # (and the shapes of a mode are searched whether or not a partition that uses them is on: the RGB counts go the same way)
    for i in range(243):
        if i not in needed or mode >= 4:
            p.seedPointsForShapeRGB[i] = 0
    for k, s in enumerate(needed):
        p.rgbShapeList[k] = s
        if mode >= 6:
            p.rgbaShapeList[k] = s
    p.rgbNumShapesToEvaluate = len(needed)
    p.rgbaNumShapesToEvaluate = len(needed) if mode >= 6 else 0
    return p


def emitted_as_asked(packed, mode, which):
    """per block: did the encoder emit the one candidate the plan left?"""
    import block_fields as F
    m = F.bc7_mode(packed)
    if mode in (0, 1, 2, 3, 7):
        return (m == mode) & (F.bc7_partition(packed) == which)
    if mode == 6:
        return m == 6
    if mode == 4:
        return (m == 4) & (F.bc7_rotation(packed) == which >> 1) & (F.bc7_index_selector(packed) == (which & 1))
    return (m == 5) & (F.bc7_rotation(packed) == which)


def rgb_modes_allowed(blocks):
    """per block: does its group of eight allow the RGB modes 0-3 (some block of the group has no alpha below 251;
    BC67.cpp:1069-1078)?"""
    blocks = np.asarray(blocks)
    ok = (blocks[:, :, 3].min(1) > 250).reshape(-1, 8).any(1)
    return np.repeat(ok, 8)


def _bytes(s):
    return np.frombuffer(s.tobytes(), np.uint8).copy()


def reached_errors(orc, blocks, opt, rcp, threads=16, cands=None):
    """reference B: E[(mode, which)] = (error per block in float64, emitted-as-asked per block, packed bytes), each
    candidate encoded on its own by the C restatement with the blocks in their groups"""
    out = {}
    ob = _bytes(opt)
    for mode, which in (cands if cands is not None else candidates()):
        packed = orc.encode_bc7(blocks, ob, _bytes(single_candidate_plan(mode, which)), rcp, threads=threads)
        out[(mode, which)] = (block_error(blocks, decode_bc7(packed), opt), emitted_as_asked(packed, mode, which), packed)
    return out
