"""numpy restatement of the mip kernels wider than 2x2 (include/cvtt_mi355x.h, "mip chains", CVTTMI_MIP_KERNEL_* and
CVTTMI_MIP_WRAP_*): the reference of the mip kernel tests.  A helper, not a test module; it does not import the package.  The
2x2 rules are mip_ref's and mip_filter_ref's.  Images are (H, W, 4) arrays, uint8 (RGBA8) or int8 (RGBA8_SNORM); a word is the
`filter` value of the C calls: rule | kernel | wrap."""
import math

import numpy as np

import mip_filter_ref
import mip_ref

BOX, SRGB, NORMAL = 0, 1, 2
KERNELS = {"triangle": 0x10, "mitchell": 0x20, "lanczos3": 0x30, "kaiser": 0x40}
WRAPS = {"clamp": 0, "repeat": 0x200, "mirror": 0x400}
RADIUS = {"triangle": 1, "mitchell": 2, "lanczos3": 3, "kaiser": 3}
KERNEL_MASK, WRAP_MASK = 0xF0, 0x600
ONE = 16384


def _sinc(x):
    return 1.0 if x == 0.0 else math.sin(math.pi * x) / (math.pi * x)


def _i0(x):
    total, term, k = 1.0, 1.0, 0
    while term > 1e-17 * total:
        k += 1
        term *= (x / (2.0 * k)) ** 2
        total += term
    return total


def _weight(kernel, t):
    a = abs(t)
    if kernel == "triangle":
        return max(0.0, 1.0 - a)
    if kernel == "mitchell":
        b = c = 1.0 / 3.0
        if a < 1.0:
            return ((12 - 9 * b - 6 * c) * a ** 3 + (-18 + 12 * b + 6 * c) * a ** 2 + (6 - 2 * b)) / 6.0
        if a < 2.0:
            return ((-b - 6 * c) * a ** 3 + (6 * b + 30 * c) * a ** 2 + (-12 * b - 48 * c) * a + (8 * b + 24 * c)) / 6.0
        return 0.0
    if a >= 3.0:
        return 0.0
    if kernel == "lanczos3":
        return _sinc(t) * _sinc(t / 3.0)
    assert kernel == "kaiser"
    return _sinc(t) * _i0(4.0 * math.sqrt(1.0 - (t / 3.0) ** 2)) / _i0(4.0)


def kernel_name(word):
    """the name of a word's kernel (a name passes through); None for kernel 0"""
    if isinstance(word, str):
        return word
    return {v: k for k, v in KERNELS.items()}.get(word & KERNEL_MASK)


def float_taps(kernel):
    """the n = 4 R weights at t_k = (k - n/2 + 0.5) / 2 in float64, divided by their sum"""
    n = 4 * RADIUS[kernel_name(kernel)]
    w = np.array([_weight(kernel_name(kernel), (k - n / 2 + 0.5) / 2.0) for k in range(n)], np.float64)
    return w / math.fsum(w)


def taps(kernel, split=True):
    """the Q14 table: floor(16384 w + 0.5), what is missing to 16384 split between the two central taps"""
    w = np.floor(ONE * float_taps(kernel) + 0.5).astype(np.int64)
    if split:
        rest = ONE - int(w.sum())
        assert rest % 2 == 0
        w[len(w) // 2 - 1] += rest // 2
        w[len(w) // 2] += rest // 2
    return w


def wrap_index(i, n, wrap):
    """source coordinates i (any integers) -> 0 .. n - 1 under a wrap mode (a name or its flag)"""
    wrap = WRAPS.get(wrap, wrap)
    i = np.asarray(i, np.int64)
    if wrap == WRAPS["repeat"]:
        return i % n
    if wrap == WRAPS["mirror"]:
        m = i % (2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    assert wrap == 0
    return np.clip(i, 0, n - 1)


def footprint(size, ntaps, wrap):
    """(max(1, size >> 1), ntaps) source coordinates: tap k of output x reads 2x + 1 - ntaps/2 + k, wrapped"""
    out = max(1, size >> 1)
    return wrap_index(2 * np.arange(out)[:, None] + 1 - ntaps // 2 + np.arange(ntaps)[None, :], size, wrap)


def _pass(v, idx, w, axis):
    """sum over k of w[k] * v[idx[:, k]] along `axis` (0 = rows, 1 = columns), int64"""
    acc = 0
    for k in range(len(w)):
        acc = acc + int(w[k]) * np.take(v, idx[:, k], axis=axis)
    return acc


def _fits(a):
    assert np.abs(a).max() < 1 << 31  # what the device holds in int32
    return a


def _two_pass(v, w, ix, iy, shift):
    """horizontal pass, h' = (h + half) >> shift, vertical pass: the sum s, int64 (checked against int32)"""
    h = _fits(_pass(v, ix, w, 1))
    hp = (h + (1 << (shift - 1))) >> shift
    return _fits(_pass(hp, iy, w, 0))


def normal_sums(img, word):
    """S_c of the NORMAL rule: (h', w', 3) int64"""
    w = taps(kernel_name(word))
    v = img.astype(np.int64)[..., :3]
    x = np.maximum(v, -127) if img.dtype == np.int8 else 2 * v - 255
    ix, iy = footprint(img.shape[1], len(w), word & WRAP_MASK), footprint(img.shape[0], len(w), word & WRAP_MASK)
    return (_two_pass(x, w, ix, iy, 10) + 128) >> 8


def downsample(img, word):
    """one level under `word` (rule | kernel | wrap, kernel not 0)"""
    rule, wrap = word & ~(KERNEL_MASK | WRAP_MASK), word & WRAP_MASK
    w = taps(kernel_name(word))
    assert rule in (BOX, SRGB, NORMAL) and img.dtype in (np.uint8, np.int8) and (img.dtype == np.uint8 or rule != SRGB)
    signed = img.dtype == np.int8
    lo, hi = (-128, 127) if signed else (0, 255)
    hgt, wid = img.shape[:2]
    ix, iy = footprint(wid, len(w), wrap), footprint(hgt, len(w), wrap)
    v = img.astype(np.int64)
    plain = np.clip((_two_pass(v, w, ix, iy, 10) + (1 << 17)) >> 18, lo, hi)
    out = plain.copy()
    if rule == SRGB:
        s = _two_pass(mip_filter_ref.T.astype(np.int64)[img[..., :3]], w, ix, iy, 14)
        out[..., :3] = mip_filter_ref.encode(np.clip((_fits(s + (1 << 11))) >> 12, 0, 4 * 65535))
    elif rule == NORMAL:
        S = normal_sums(img, word)
        assert np.abs(S).max() < 1 << 20
        f = S.astype(np.float32)
        length = np.sqrt((f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]) + f[..., 2] * f[..., 2])
        zero = (S == 0).all(axis=-1)
        q = f / np.where(zero, np.float32(1), length)[..., None]
        assert q.dtype == np.float32 and length.dtype == np.float32
        if signed:
            r = np.clip(np.floor(q * np.float32(127.0) + np.float32(0.5)).astype(np.int64), -127, 127)
        else:
            r = np.clip(np.floor(q * np.float32(127.5) + np.float32(128.0)).astype(np.int64), 0, 255)
        out[..., :3] = np.where(zero[..., None], plain[..., :3], r)
    return out.astype(img.dtype)


def chain(img, word, levels=None):
    """[level 0 = img, level 1, ...]: every level from the rounded one before it.  A word without kernel bits is the 2x2 rule
    of mip_filter_ref."""
    if word & KERNEL_MASK == 0:
        return mip_filter_ref.chain(img, word, levels)
    out = [img]
    for _ in range((len(mip_ref.level_sizes(img.shape[1], img.shape[0])) if levels is None else levels) - 1):
        out.append(downsample(out[-1], word))
    return out


def planted_image(kernel, w, h, dtype=np.uint8, seed=1):
    """random (h, w, 4) image of a kernel's hardest footprints, as many as the size has room for; returns (image, spots):
    spots[0], spots[1] = (x, y, byte): the footprint of output texel (x, y) holds the largest value under every positive tap and
        the smallest under every negative one (rows under a negative vertical tap the other way round), and the reverse -- the
        largest |h| and |s| there are; every channel of the texel comes out as `byte`, by the last clamp
    spots[2] = (x, y, None): the colour channels of the footprint's columns k and n - 1 - k are v and 255 - v (int8: v and -v),
        so the NORMAL rule's three sums are all zero there"""
    rng = np.random.default_rng(seed + w * 131 + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8).view(dtype)
    w_ = taps(kernel)
    n = len(w_)
    lo, hi = (0, 255) if dtype == np.uint8 else (-128, 127)
    spots = []
    for (x, y), sign in (((n // 4 + 1, n // 4 + 1), 1), ((n // 4 + 2 + n // 2, n // 4 + 1), -1), ((n // 4 + 1, n // 4 + 2 + n // 2), 0)):
        c0, r0 = 2 * x + 1 - n // 2, 2 * y + 1 - n // 2
        if c0 + n > w or r0 + n > h:
            continue
        if sign:
            col = np.where(sign * w_ > 0, hi, lo)
            block = np.where((w_ > 0)[:, None], col[None, :], (hi + lo) - col[None, :])
            img[r0: r0 + n, c0: c0 + n] = block[..., None].astype(dtype)
            spots.append((x, y, hi if sign > 0 else lo))
        else:
            left = img[r0: r0 + n, c0: c0 + n // 2, :3].astype(np.int64)
            if dtype == np.int8:
                left = np.maximum(left, -127)
                img[r0: r0 + n, c0: c0 + n // 2, :3] = left.astype(dtype)
            img[r0: r0 + n, c0 + n // 2: c0 + n, :3] = ((-left if dtype == np.int8 else 255 - left)[:, ::-1]).astype(dtype)
            spots.append((x, y, None))
    return img, spots


# ---- plain float64 arithmetic: the independent anchor (unquantised weights, no intermediate rounding) ----

def float64_level(img, word):
    """channels 0..2 of one level of a uint8 image under the plain rule or SRGB, as codes; channel 3 under the plain rule"""
    rule, wrap = word & ~(KERNEL_MASK | WRAP_MASK), word & WRAP_MASK
    w = float_taps(word)
    hgt, wid = img.shape[:2]
    ix, iy = footprint(wid, len(w), wrap), footprint(hgt, len(w), wrap)
    v = img.astype(np.float64)
    if rule == SRGB:
        v[..., :3] = mip_filter_ref.lin(v[..., :3] / 255.0)
    h = sum(w[k] * v[:, ix[:, k]] for k in range(len(w)))
    s = sum(w[k] * h[iy[:, k]] for k in range(len(w)))
    if rule == SRGB:
        s[..., :3] = 255.0 * mip_filter_ref._oetf(np.clip(s[..., :3], 0.0, 1.0))
    return np.clip(np.floor(s + 0.5), 0, 255).astype(np.int64)
