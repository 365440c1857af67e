"""numpy restatement of the resize rule (include/cvtt_mi355x.h, "resize"): the reference of the resize tests.  A helper, not a
test module; it does not import the package.  The weight functions, the wrap modes, the sRGB tables and the float64 transfer
functions are mip_resample_ref's and mip_filter_ref's.  Images are (H, W, 4) arrays, uint8 (RGBA8) or int8 (RGBA8_SNORM)."""
import math

import numpy as np

import mip_filter_ref
import mip_resample_ref as M

BOX, SRGB, NORMAL = M.BOX, M.SRGB, M.NORMAL
KERNELS = dict(M.KERNELS, box=0)
RADIUS2 = {"box": 1, "triangle": 2, "mitchell": 4, "lanczos3": 6, "kaiser": 6}  # 2 R
ONE = M.ONE


def tap_count(src, dst, kernel):
    big = max(src, dst)
    return -(-big // dst) + 1 if kernel == "box" else -(-(RADIUS2[kernel] * big) // dst)


def first_taps(src, dst, kernel):
    """first[x], unwrapped"""
    big = max(src, dst)
    L = (2 * np.arange(dst, dtype=np.int64) + 1) * src - dst - RADIUS2[kernel] * big
    return (L + dst) // (2 * dst) if kernel == "box" else L // (2 * dst) + 1


def float_weights(src, dst, kernel):
    """(dst, n) float64: the weights of every row divided by their sum, unquantised (box: the overlaps / (2 big))"""
    big, n, first = max(src, dst), tap_count(src, dst, kernel), first_taps(src, dst, kernel)
    w = np.zeros((dst, n), np.float64)
    for x in range(dst):
        centre = (2 * x + 1) * src - dst
        if src == dst:  # the image itself, for every kernel (Mitchell's K(0) = 8/9 would blur it)
            w[x, x - int(first[x])] = 1.0
            continue
        for k in range(n):
            j = int(first[x]) + k
            if kernel == "box":
                w[x, k] = max(0, min(centre + big, 2 * dst * j + dst) - max(centre - big, 2 * dst * j - dst)) / float(2 * big)
            else:
                w[x, k] = M._weight(kernel, float(2 * dst * j - centre) / float(2 * big))
        if kernel != "box":
            total = 0.0
            for k in range(n):
                total += w[x, k]
            w[x] = w[x] / total
    return w


def positive_sum(q):
    """P: the largest sum of positive taps over the rows of a table"""
    return int(np.maximum(np.asarray(q, np.int64), 0).sum(axis=1).max())


def guard_holds(q):
    P = positive_sum(q)
    return 65535 * P < 1 << 31 and ((65535 * P + 8192) >> 14) * (2 * P - 16384) < 1 << 31


def table(src, dst, kernel):
    """(first, q): first[x] int64, q[x, k] int64 Q14, every row summing to 16384; asserts the int32 guard"""
    big, n, first = max(src, dst), tap_count(src, dst, kernel), first_taps(src, dst, kernel)
    q = np.zeros((dst, n), np.int64)
    w = float_weights(src, dst, kernel) if kernel != "box" else None
    for x in range(dst):
        if src == dst:
            q[x, x - int(first[x])] = ONE
            continue
        if kernel == "box":
            centre = (2 * x + 1) * src - dst
            row = []
            for k in range(n):
                j = int(first[x]) + k
                o = max(0, min(centre + big, 2 * dst * j + dst) - max(centre - big, 2 * dst * j - dst))
                row.append((2 * ONE * o + 2 * big) // (4 * big))
            assert sum(max(0, min(centre + big, 2 * dst * (int(first[x]) + k) + dst) - max(centre - big, 2 * dst * (int(first[x]) + k) - dst))
                       for k in range(n)) == 2 * big
        else:
            row = [int(math.floor(ONE * w[x, k] + 0.5)) for k in range(n)]
        row = np.array(row, np.int64)
        rest = ONE - int(row.sum())
        top = np.flatnonzero(row == row.max())
        each = rest // len(top) if rest >= 0 else -((-rest) // len(top))  # towards zero
        row[top] += each
        row[top[0]] += rest - each * len(top)
        assert row.sum() == ONE
        q[x] = row
    assert guard_holds(q), (src, dst, kernel, positive_sum(q))
    return first, q


def _rows(v, idx, q, axis):
    """sum over k of q[:, k] * v[idx[:, k]] along `axis` (0 = rows, 1 = columns), every output with its own weight row"""
    acc = 0
    for k in range(q.shape[1]):
        weight = q[:, k][:, None, None] if axis == 0 else q[:, k][None, :, None]
        acc = acc + weight * np.take(v, idx[:, k], axis=axis)
    return acc


def _two_pass(v, tx, ty, ix, iy, shift):
    h = M._fits(_rows(v, ix, tx, 1))
    hp = (h + (1 << (shift - 1))) >> shift
    return M._fits(_rows(hp, iy, ty, 0))


def resize(img, width, height, kernel="lanczos3", rule=BOX, wrap="clamp", tables=None):
    """(H, W, 4) -> (height, width, 4) under the rule of the header.  tables = ((first_x, q_x), (first_y, q_y)): the tables to
    use (what cvttmi_resize_taps returned) instead of this module's own"""
    assert rule in (BOX, SRGB, NORMAL) and img.dtype in (np.uint8, np.int8) and (img.dtype == np.uint8 or rule != SRGB)
    hgt, wid = img.shape[:2]
    (fx, qx), (fy, qy) = tables if tables is not None else (table(wid, width, kernel), table(hgt, height, kernel))
    fx, qx, fy, qy = (np.asarray(a, np.int64) for a in (fx, qx, fy, qy))
    ix = M.wrap_index(fx[:, None] + np.arange(qx.shape[1])[None], wid, wrap)
    iy = M.wrap_index(fy[:, None] + np.arange(qy.shape[1])[None], hgt, wrap)
    signed = img.dtype == np.int8
    lo, hi = (-128, 127) if signed else (0, 255)
    v = img.astype(np.int64)
    plain = np.clip((_two_pass(v, qx, qy, ix, iy, 10) + (1 << 17)) >> 18, lo, hi)
    out = plain.copy()
    if rule == SRGB:
        s = _two_pass(mip_filter_ref.T.astype(np.int64)[img[..., :3]], qx, qy, ix, iy, 14)
        out[..., :3] = mip_filter_ref.encode(np.clip(M._fits(s + (1 << 11)) >> 12, 0, 4 * 65535))
    elif rule == NORMAL:
        x = np.maximum(v[..., :3], -127) if signed else 2 * v[..., :3] - 255
        S = (_two_pass(x, qx, qy, ix, iy, 10) + 128) >> 8
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


def float64_resize(img, width, height, kernel, rule=BOX, wrap="clamp"):
    """plain float64 convolution, unquantised weights, no intermediate rounding: the independent anchor.  uint8 images, the plain
    rule or SRGB (channel 3 always plain), as codes"""
    hgt, wid = img.shape[:2]
    wx, wy = float_weights(wid, width, kernel), float_weights(hgt, height, kernel)
    ix = M.wrap_index(first_taps(wid, width, kernel)[:, None] + np.arange(wx.shape[1])[None], wid, wrap)
    iy = M.wrap_index(first_taps(hgt, height, kernel)[:, None] + np.arange(wy.shape[1])[None], hgt, wrap)
    v = img.astype(np.float64)
    if rule == SRGB:
        v[..., :3] = mip_filter_ref.lin(v[..., :3] / 255.0)
    s = _rows(_rows(v, ix, wx, 1), iy, wy, 0)
    if rule == SRGB:
        s[..., :3] = 255.0 * mip_filter_ref._oetf(np.clip(s[..., :3], 0.0, 1.0))
    return np.clip(np.floor(s + 0.5), 0, 255).astype(np.int64)


def planted_image(kernel, w, h, width, height, dtype=np.uint8, seed=1):
    """random (h, w, 4) image for a resize to width x height with the tables' hardest footprints planted, in the way of
    mip_resample_ref.planted_image; returns (image, spots).  The footprint of an output texel is the rows first_y[y] .. + ny - 1 by
    the columns first_x[x] .. + nx - 1; only footprints that lie inside the image and do not overlap are planted.
    spots[0], spots[1] = (x, y, byte): the largest value under every positive tap and the smallest under every negative one
        (rows under a negative vertical tap the other way round), and the reverse: the largest |h| and |s| these rows reach;
        every channel of the texel comes out as `byte`, by the last clamp
    spots[2] = (x, y, None), only where some column's weight row is symmetric (its non-zero taps a palindrome of even length, as every
        row is at exactly half): the colour channels of the columns under taps k and m - 1 - k of them are v and 255 - v (int8: v and
        -v), so the NORMAL rule's three sums are all zero"""
    rng = np.random.default_rng(seed + w * 131 + h + 7 * width + 3 * height)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8).view(dtype)
    (fx, qx), (fy, qy) = table(w, width, kernel), table(h, height, kernel)
    nx, ny = qx.shape[1], qy.shape[1]
    lo, hi = (0, 255) if dtype == np.uint8 else (-128, 127)
    inside = [(x, y) for y in range(height) for x in range(width)
              if fx[x] >= 0 and fx[x] + nx <= w and fy[y] >= 0 and fy[y] + ny <= h]
    taken, spots = [], []

    def free(x, y):
        box = (fx[x], fx[x] + nx, fy[y], fy[y] + ny)
        if any(box[0] < t[1] and t[0] < box[1] and box[2] < t[3] and t[2] < box[3] for t in taken):
            return False
        taken.append(box)
        return True
    for sign in (1, -1, 0):
        for x, y in inside:
            nz = np.flatnonzero(qx[x])
            a, m = int(nz[0]), int(nz[-1]) + 1 - int(nz[0])  # the taps that weigh: columns a .. a + m - 1 of the footprint
            if sign == 0 and not ((qx[x][a: a + m] == qx[x][a: a + m][::-1]).all() and m % 2 == 0):
                continue
            if not free(x, y):
                continue
            c0, r0 = int(fx[x]), int(fy[y])
            if sign:
                col = np.where(sign * qx[x] > 0, hi, lo)
                block = np.where((qy[y] > 0)[:, None], col[None, :], (hi + lo) - col[None, :])
                img[r0: r0 + ny, c0: c0 + nx] = block[..., None].astype(dtype)
                spots.append((x, y, hi if sign > 0 else lo))
            else:
                c0 += a
                left = img[r0: r0 + ny, c0: c0 + m // 2, :3].astype(np.int64)
                if dtype == np.int8:
                    left = np.maximum(left, -127)
                    img[r0: r0 + ny, c0: c0 + m // 2, :3] = left.astype(dtype)
                img[r0: r0 + ny, c0 + m // 2: c0 + m, :3] = ((-left if dtype == np.int8 else 255 - left)[:, ::-1]).astype(dtype)
                spots.append((x, y, None))
            break
    return img, spots
