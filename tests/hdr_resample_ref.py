"""numpy float32 restatement of RGBA16F under a mip kernel and in a resize (include/cvtt_mi355x.h, "RGBA16F under a kernel"): the
reference of the HDR resample tests.  A helper, not a test module; it does not import the package.  Footprints, taps, first taps
and wraps are mip_resample_ref's and resize_ref's.  Images are (H, W, 4) arrays of half bit patterns (uint16; float16 is taken
too); results are uint16.  Every product and every sum is one numpy float32 operation, so each is rounded on its own, as the
rule says; the intermediates are asserted to be float32."""
import numpy as np

import mip_ref
import mip_resample_ref as M
import resize_ref as R

NONNEGATIVE, SIGNED = 0x1000, 0x2000
HDR = {"nonnegative": NONNEGATIVE, "signed": SIGNED}
RANGE_MASK = NONNEGATIVE | SIGNED
MAX = 65504.0
FINITE_MAX_BITS = 0x7BFF  # the bit pattern of 65504


def bits(img):
    img = np.asarray(img)
    assert img.dtype in (np.uint16, np.float16)
    return img.view(np.uint16)


def low(hdr):
    """the lower clamp of a range (a name or its flag)"""
    flag = HDR.get(hdr, hdr)
    assert flag in (NONNEGATIVE, SIGNED)
    return -MAX if flag == SIGNED else 0.0


def _f32(a):
    assert a.dtype == np.float32
    return a


def _rows(v, idx, q, axis):
    """s = +0; s = s + (w_k * v[idx[:, k]]) in index order along `axis` (0 = rows, 1 = columns), every output with its own weight
    row q[x] (Q14 integers; w = q * 2^-14 is exact)"""
    w = _f32(np.asarray(q, np.int64).astype(np.float32) * np.float32(2.0 ** -14))
    assert (w.astype(np.float64) * 16384 == np.asarray(q)).all()
    acc = None
    for k in range(w.shape[1]):
        weight = w[:, k][:, None, None] if axis == 0 else w[:, k][None, :, None]
        term = _f32(weight * np.take(v, idx[:, k], axis=axis))
        acc = _f32((np.zeros_like(term) if acc is None else acc) + term)
    return acc


def finish(s, lo, dtype=np.float32):
    """the clamp by comparisons (a NaN passes both) and the one rounding to half"""
    assert s.dtype == dtype
    lo, hi = dtype(lo), dtype(MAX)
    c = np.where(s < lo, lo, np.where(s > hi, hi, s))
    assert c.dtype == dtype
    return c.astype(np.float16).view(np.uint16)


def two_pass(img, qx, ix, qy, iy, lo):
    with np.errstate(all="ignore"):
        v = _f32(bits(img).view(np.float16).astype(np.float32))
        return finish(_rows(_rows(v, ix, qx, 1), iy, qy, 0), lo)


def _mip_tables(img, word):
    w = M.taps(M.kernel_name(word & M.KERNEL_MASK))
    hgt, wid = img.shape[:2]
    ix, iy = M.footprint(wid, len(w), word & M.WRAP_MASK), M.footprint(hgt, len(w), word & M.WRAP_MASK)
    return np.tile(w, (ix.shape[0], 1)), ix, np.tile(w, (iy.shape[0], 1)), iy


def downsample(img, word):
    """one level under `word` = kernel | wrap | one range flag (the rule field is 0, the plain rule)"""
    assert word & ~(M.KERNEL_MASK | M.WRAP_MASK | RANGE_MASK) == 0 and word & M.KERNEL_MASK
    qx, ix, qy, iy = _mip_tables(img, word)
    return two_pass(img, qx, ix, qy, iy, low(word & RANGE_MASK))


def chain(img, word, levels=None):
    """[level 0 = the image's bits, level 1, ...]: every level from the rounded one before it"""
    out = [bits(img)]
    for _ in range((len(mip_ref.level_sizes(img.shape[1], img.shape[0])) if levels is None else levels) - 1):
        out.append(downsample(out[-1], word))
    return out


def _resize_tables(img, width, height, kernel, wrap, tables=None):
    hgt, wid = img.shape[:2]
    (fx, qx), (fy, qy) = tables if tables is not None else (R.table(wid, width, kernel), R.table(hgt, height, kernel))
    fx, qx, fy, qy = (np.asarray(a, np.int64) for a in (fx, qx, fy, qy))
    ix = M.wrap_index(fx[:, None] + np.arange(qx.shape[1])[None], wid, wrap)
    iy = M.wrap_index(fy[:, None] + np.arange(qy.shape[1])[None], hgt, wrap)
    return qx, ix, qy, iy


def resize(img, width, height, kernel="lanczos3", hdr="nonnegative", wrap="clamp", tables=None):
    """(H, W, 4) -> (height, width, 4) under a range (a name of HDR or its flag); tables as for resize_ref.resize"""
    qx, ix, qy, iy = _resize_tables(img, width, height, kernel, wrap, tables)
    return two_pass(img, qx, ix, qy, iy, low(hdr))


# ---- plain float64 convolution with the same Q14 weights, the same clamp and one final rounding to half: the anchor ----

def _float64(img, qx, ix, qy, iy, lo):
    v = bits(img).view(np.float16).astype(np.float64)
    h = sum((qx[:, k] / 16384.0)[None, :, None] * np.take(v, ix[:, k], axis=1) for k in range(qx.shape[1]))
    s = sum((qy[:, k] / 16384.0)[:, None, None] * np.take(h, iy[:, k], axis=0) for k in range(qy.shape[1]))
    return finish(s, lo, np.float64)


def float64_level(img, word):
    return _float64(img, *_mip_tables(img, word), low(word & RANGE_MASK))


def float64_resize(img, width, height, kernel, hdr, wrap="clamp"):
    return _float64(img, *_resize_tables(img, width, height, kernel, wrap), low(hdr))


def code_distance(a, b):
    """how many half codes apart two arrays of finite half bit patterns are, element by element (+0 and -0 are one step apart)"""
    def line(u):
        u = u.astype(np.int64)
        return np.where(u & 0x8000, -(u & 0x7FFF) - 1, u)
    return np.abs(line(bits(a)) - line(bits(b)))


# ---- inputs ----

def random_finite(rng, shape):
    """uniformly random finite half bit patterns of both signs"""
    u = rng.integers(0, 1 << 16, shape, dtype=np.uint16)
    return np.where((u & 0x7C00) == 0x7C00, u & 0x83FF, u).astype(np.uint16)


def planted_image(kernel, w, h, seed=1):
    """random finite (h, w, 4) image with a kernel's two hardest footprints planted where the size has room, in the way of
    mip_resample_ref.planted_image; returns (bits, spots), spots = [(x, y, sign)]: under sign +1 the footprint of output texel (x, y)
    holds +65504 under every positive tap and -65504 under every negative one (rows under a negative vertical tap the other way
    round), so the sum is far above 65504; under -1 the reverse, far below -65504"""
    rng = np.random.default_rng(seed + w * 131 + h)
    img = random_finite(rng, (h, w, 4))
    w_ = M.taps(kernel)
    n = len(w_)
    spots = []
    for (x, y), sign in (((n // 4 + 1, n // 4 + 1), 1), ((n // 4 + 2 + n // 2, n // 4 + 1), -1)):
        c0, r0 = 2 * x + 1 - n // 2, 2 * y + 1 - n // 2
        if c0 + n > w or r0 + n > h:
            continue
        col = np.where(sign * w_ > 0, MAX, -MAX)
        block = np.where((w_ > 0)[:, None], col[None, :], -col[None, :]).astype(np.float16)
        img[r0: r0 + n, c0: c0 + n] = block.view(np.uint16)[..., None]
        spots.append((x, y, sign))
    return img, spots
