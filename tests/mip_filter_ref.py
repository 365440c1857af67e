"""numpy restatement of the mip filters beyond the box (include/cvtt_mi355x.h, "mip chains", CVTTMI_MIP_FILTER_*): the reference
of the mip filter tests.  A helper, not a test module; it does not import the package.  Geometry and the box rule are mip_ref's.
Images are (H, W, 4) arrays, uint8 (RGBA8) or int8 (RGBA8_SNORM).  Filters are named as Context.build_mips names them."""
import numpy as np

import mip_ref

BOX, SRGB, NORMAL, ALPHA_WEIGHTED = 0, 1, 2, 0x100
FILTERS = {"box": BOX, "srgb": SRGB, "normal": NORMAL, "box+alpha": BOX | ALPHA_WEIGHTED, "srgb+alpha": SRGB | ALPHA_WEIGHTED}


def lin(e):
    """the sRGB EOTF in float64"""
    e = np.asarray(e, np.float64)
    return np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4)


def tables():
    """T[v], v = 0..255 (uint16) and U[k], k = 1..255 (uint32, U[k] at index k - 1)"""
    t = np.floor(65535.0 * lin(np.arange(256) / 255.0) + 0.5).astype(np.uint16)
    u = np.ceil(4.0 * 65535.0 * lin((np.arange(1, 256) - 0.5) / 255.0)).astype(np.uint32)
    return t, u


T, U = tables()


def encode(s):
    """the number of k with s >= U[k]"""
    return np.searchsorted(U, np.asarray(s, np.int64), side="right")


def quads(img):
    """the four (h', w', 4) int64 arrays a, b, c, d a level is made from: mip_ref.downsample's geometry"""
    h, w = img.shape[:2]
    y0, x0 = 2 * np.arange(max(1, h >> 1)), 2 * np.arange(max(1, w >> 1))
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    return [v.astype(np.int64) for v in (img[y0][:, x0], img[y0][:, x1], img[y1][:, x0], img[y1][:, x1])]


def downsample(img, filt):
    """one level under filter `filt` (a name or a CVTTMI_MIP_FILTER_* value)"""
    filt = FILTERS.get(filt, filt)
    box = mip_ref.downsample(img)
    if filt == BOX:
        return box
    assert img.dtype in (np.uint8, np.int8) and (img.dtype == np.uint8 or filt == NORMAL)
    q = quads(img)
    out = box.copy()  # channel 3, and whatever falls back to the box rule
    if filt == NORMAL:
        x = [2 * v[..., :3] - 255 if img.dtype == np.uint8 else np.maximum(v[..., :3], -127) for v in q]
        s = x[0] + x[1] + x[2] + x[3]
        qq = (s * s).sum(axis=-1)
        assert qq.max() < 1 << 24
        length = np.sqrt(np.where(qq == 0, 1, qq).astype(np.float32))  # float32 sqrt and divide: IEEE, correctly rounded
        unit = s.astype(np.float32) / length[..., None]
        if img.dtype == np.uint8:
            r = np.clip(np.floor(unit * np.float32(127.5) + np.float32(128.0)).astype(np.int64), 0, 255)
        else:
            r = np.clip(np.floor(unit * np.float32(127.0) + np.float32(0.5)).astype(np.int64), -127, 127)
        assert unit.dtype == np.float32
        out[..., :3] = np.where((qq == 0)[..., None], box[..., :3], r.astype(img.dtype))
        return out
    srgb, weighted = bool(filt & SRGB), bool(filt & ALPHA_WEIGHTED)
    assert filt & ~(SRGB | ALPHA_WEIGHTED) == 0
    v = [T[t[..., :3]].astype(np.int64) if srgb else t[..., :3] for t in q]
    plain = v[0] + v[1] + v[2] + v[3]
    if weighted:
        al = [t[..., 3:4] for t in q]
        a = al[0] + al[1] + al[2] + al[3]
        n = v[0] * al[0] + v[1] * al[1] + v[2] * al[2] + v[3] * al[3]
        a1 = np.where(a == 0, 1, a)
        if srgb:
            assert (4 * n + (a >> 1)).max() < 1 << 32
            r = encode(np.where(a == 0, plain, (4 * n + (a >> 1)) // a1))
        else:
            r = np.where(a == 0, box[..., :3], (2 * n + a) // (2 * a1))
    else:
        r = encode(plain)
    out[..., :3] = r.astype(np.uint8)
    return out


def chain(img, filt, levels=None):
    """[level 0 = img, level 1, ...]: every level from the rounded one before it"""
    out = [img]
    for _ in range((len(mip_ref.level_sizes(img.shape[1], img.shape[0])) if levels is None else levels) - 1):
        out.append(downsample(out[-1], filt))
    return out


# ---- plain float64 arithmetic: the independent anchor of the rules above (a, b, c, d: (..., 4) arrays of one quad each) ----

def _oetf(x):
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.maximum(x, 1e-30) ** (1 / 2.4) - 0.055)


def float64_srgb(a, b, c, d, weighted=False):
    """mean of lin (alpha-weighted if asked and the alphas do not sum to 0), inverse OETF, round to nearest"""
    t = [lin(v[..., :3] / 255.0) for v in (a, b, c, d)]
    w = [v[..., 3:4].astype(np.float64) for v in (a, b, c, d)]
    tot = w[0] + w[1] + w[2] + w[3]
    if not weighted:
        w, tot = [1.0] * 4, 4.0
    else:
        w = [np.where(tot == 0, 1.0, x) for x in w]
        tot = np.where(tot == 0, 4.0, tot)
    mean = (t[0] * w[0] + t[1] * w[1] + t[2] * w[2] + t[3] * w[3]) / tot
    return np.floor(255.0 * _oetf(mean) + 0.5).astype(np.int64)


def float64_box_weighted(a, b, c, d):
    w = [v[..., 3:4].astype(np.float64) for v in (a, b, c, d)]
    tot = w[0] + w[1] + w[2] + w[3]
    w = [np.where(tot == 0, 1.0, x) for x in w]
    tot = np.where(tot == 0, 4.0, tot)
    return np.floor((a[..., :3] * w[0] + b[..., :3] * w[1] + c[..., :3] * w[2] + d[..., :3] * w[3]) / tot + 0.5).astype(np.int64)


def float64_normal(a, b, c, d):
    """RGBA8: mean of the decoded vectors, normalised, encoded as floor(n * 127.5 + 128) clamped; None where the sum is 0"""
    s = sum(2.0 * v[..., :3].astype(np.float64) - 255.0 for v in (a, b, c, d))
    length = np.sqrt((s * s).sum(axis=-1, keepdims=True))
    unit = s / np.where(length == 0, 1.0, length)
    return np.clip(np.floor(unit * 127.5 + 128.0), 0, 255).astype(np.int64), length[..., 0] != 0
