"""numpy restatement of the texture decoders and of the error measurement of csrc/decode_kernel.hip (test helper).

Written from the reconstruction rules of INTEGRATION.md ("Decoding and measuring every format"), which follow the models the
reference encoder scores its candidates with:
  BC1-BC3 colour   5/6-bit endpoints expanded by bit replication (ConvectionKernels_S3TC.cpp:52-62), interpolated with
                   IndexSelector::ReconstructLDRPrecise (ConvectionKernels_IndexSelector.h:102-112): weights 0/256/85/171
                   (c0 > c1) or 0/256/128 + transparent black (c0 <= c1, BC1 only: BC2 / BC3 colour is always four-colour,
                   and the reference's PackRGB without alpha test only emits range 4, S3TC.cpp:939-1000)
  BC2 alpha        4 bits x 17 (S3TC.cpp:306-341 packs nibbles, low nibble = even texel)
  BC3 alpha, BC4/5 the 8-level / 6-level (+0 / high terminal) ramps of PackInterpolatedAlpha (S3TC.cpp:343-715,
                   ReconstructLDRPrecise at 441 and 590; file index order 660-700); signed: Util::BiasSignedInput
                   (ConvectionKernels_Util.cpp:47-60) -- -128 reads as -127, high terminal 254 in the biased domain
  ETC1/ETC2/EAC    integer-exact: individual, differential, T, H, planar, punch-through (ETC.cpp emitters 2414-2622);
                   EAC 8-bit and R11 as QuantizeETC2Alpha reconstructs (ETC.cpp:2366-2404, input ranges 2087-2113)
  (tests/test_encoder_error_anchor.py holds all of the above but R11 to the encoder's own final per-block error, exactly)
  BC7 / BC6H       not restated here: the reference's decoders (oracle/_ref) and tests/golden/decode.npz cover them

Layouts ("a decoder writes what its encoder reads"): PixelBlockU8 (N,16,4) uint8; BC4S/BC5S PixelBlockS8 (N,16,4) int8;
BC6H PixelBlockF16 (N,16,4) int16 half bits; R11 PixelBlockScalarS16 (N,16) int16.  Texel p = 4 * row + column.
"""
import numpy as np

# name -> (format id, bytes per block, measured channel mask, PSNR peak or None)
FORMATS = {
    "bc7": (0, 16, 0xF, 255), "bc1": (1, 8, 0xF, 255), "bc6hu": (2, 16, 0x7, None), "bc6hs": (3, 16, 0x7, None),
    "etc2": (4, 8, 0x7, 255), "etc2rgb": (4, 8, 0x7, 255), "etc2rgba": (5, 16, 0xF, 255),
    "bc2": (6, 16, 0xF, 255), "bc3": (7, 16, 0xF, 255), "bc4u": (8, 8, 0x1, 255), "bc4s": (9, 8, 0x1, 254),
    "bc5u": (10, 16, 0x3, 255), "bc5s": (11, 16, 0x3, 254), "etc1": (12, 8, 0x7, 255), "etc2punchthrough": (13, 8, 0xF, 255),
    "eac": (14, 8, 0x8, 255), "r11u": (15, 8, 0x1, 2047), "r11s": (16, 8, 0x1, 2046),
}
# one name per id, in id order
NAMES = ["bc7", "bc1", "bc6hu", "bc6hs", "etc2", "etc2rgba", "bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s", "etc1",
         "etc2punchthrough", "eac", "r11u", "r11s"]

ETC1_MODIFIERS = np.array([[2, 8], [5, 17], [9, 29], [13, 42], [18, 60], [24, 80], [33, 106], [47, 183]], np.int32)
TH_DISTANCE = np.array([3, 6, 11, 16, 23, 32, 41, 64], np.int32)
# positive halves of the EAC modifier tables; index i < 4 is -(pos[i] + 1), i >= 4 is pos[i - 4] (ETC.cpp:2366-2404)
EAC_POSITIVE = np.array([
    [2, 5, 8, 14], [2, 6, 9, 12], [1, 4, 7, 12], [1, 3, 5, 12], [2, 5, 7, 11], [2, 6, 8, 10], [3, 6, 7, 10], [2, 4, 7, 10],
    [1, 5, 7, 9], [1, 4, 7, 9], [1, 3, 7, 9], [1, 4, 6, 9], [2, 3, 6, 9], [0, 1, 2, 9], [3, 5, 7, 8], [2, 4, 6, 8]], np.int32)
EAC_MODIFIERS = np.concatenate([-(EAC_POSITIVE + 1), EAC_POSITIVE], axis=1)  # (16, 8)

# ReconstructLDRPrecise weights, (g_weightReciprocals[range] * k + 64) >> 7, by the reference's linear index k
W4 = np.array([0, 85, 171, 256], np.int32)
W3 = np.array([0, 128, 256], np.int32)
W8 = np.array([0, 37, 73, 110, 146, 183, 219, 256], np.int32)
W6 = np.array([0, 51, 102, 154, 205, 256], np.int32)


def _lerp(e0, e1, w):
    return ((256 - w) * e0 + w * e1 + 128) >> 8


def _u16(b, off):
    return b[:, off].astype(np.int32) | (b[:, off + 1].astype(np.int32) << 8)


def _u32(b, off):
    return (b[:, off].astype(np.int64) | (b[:, off + 1].astype(np.int64) << 8) | (b[:, off + 2].astype(np.int64) << 16)
            | (b[:, off + 3].astype(np.int64) << 24))


def _be64(b, off):
    w = np.zeros(len(b), np.uint64)
    for i in range(8):
        w = (w << np.uint64(8)) | b[:, off + i].astype(np.uint64)
    return w


def _bits(w, shift, n):
    return ((w >> np.uint64(shift)) & np.uint64((1 << n) - 1)).astype(np.int32)


# ---- S3TC ----
def bc1_colour(b, off=0, four_colour_only=False):
    """(N,16,4) int32 RGBA of the colour half at byte `off`; returns (rgba, transparent mask)"""
    c0, c1 = _u16(b, off), _u16(b, off + 2)
    idx_word = _u32(b, off + 4)

    def expand(c):
        r, g, bl = (c >> 11) & 31, (c >> 5) & 63, c & 31
        return np.stack([(r << 3) | (r >> 2), (g << 2) | (g >> 4), (bl << 3) | (bl >> 2)], axis=1)  # (N,3)

    e0, e1 = expand(c0), expand(c1)
    four = (c0 > c1) | four_colour_only
    n = len(b)
    out = np.zeros((n, 16, 4), np.int32)
    transparent = np.zeros((n, 16), bool)
    for px in range(16):
        i = ((idx_word >> (2 * px)) & 3).astype(np.int32)
        w = np.where(four, W4[np.array([0, 3, 1, 2])[i]], W3[np.minimum(np.array([0, 2, 1, 1])[i], 2)])
        rgb = _lerp(e0, e1, w[:, None])
        t = ~four & (i == 3)
        out[:, px, :3] = np.where(t[:, None], 0, rgb)
        out[:, px, 3] = np.where(t, 0, 255)
        transparent[:, px] = t
    return out, transparent


def interpolated_alpha(b, off=0, signed=False):
    """(N,16) int32 of a BC3-alpha / BC4 / BC5 channel block: 0..255, or -127..127 when signed"""
    if signed:
        r0 = b[:, off].astype(np.int8).astype(np.int32)
        r1 = b[:, off + 1].astype(np.int8).astype(np.int32)
        full = r0 > r1
        e0, e1 = np.maximum(r0, -127) + 127, np.maximum(r1, -127) + 127
        high = 254
    else:
        e0, e1 = b[:, off].astype(np.int32), b[:, off + 1].astype(np.int32)
        full = e0 > e1
        high = 255
    bits = np.zeros(len(b), np.int64)
    for i in range(6):
        bits |= b[:, off + 2 + i].astype(np.int64) << (8 * i)
    out = np.zeros((len(b), 16), np.int32)
    for px in range(16):
        i = ((bits >> (3 * px)) & 7).astype(np.int32)
        k8 = np.array([0, 7, 1, 2, 3, 4, 5, 6])[i]
        k6 = np.array([0, 5, 1, 2, 3, 4, 0, 0])[i]
        v8 = _lerp(e0, e1, W8[k8])
        v6 = np.where(i == 6, 0, np.where(i == 7, high, _lerp(e0, e1, W6[k6])))
        out[:, px] = np.where(full, v8, v6)
    return out - 127 if signed else out


def explicit_alpha(b, off=0):
    out = np.zeros((len(b), 16), np.int32)
    for px in range(16):
        out[:, px] = ((b[:, off + px // 2].astype(np.int32) >> (4 * (px & 1))) & 15) * 17
    return out


# ---- ETC ----
def _clamp255(v):
    return np.clip(v, 0, 255)


def etc_colour(b, off=0, punchthrough=False):
    """(N,16,4) int32 RGBA of an ETC1 / ETC2 RGB / ETC2 punch-through colour block at byte `off` (big-endian 64-bit word)."""
    w = _be64(b, off)
    n = len(b)
    diffbit = _bits(w, 33, 1).astype(bool)
    flip = _bits(w, 32, 1).astype(bool)
    differential = np.ones(n, bool) if punchthrough else diffbit
    opaque = diffbit if punchthrough else np.ones(n, bool)

    def sext3(v):
        return np.where(v >= 4, v - 8, v)

    rb, gb, bb = _bits(w, 59, 5), _bits(w, 51, 5), _bits(w, 43, 5)
    r2, g2, b2 = rb + sext3(_bits(w, 56, 3)), gb + sext3(_bits(w, 48, 3)), bb + sext3(_bits(w, 40, 3))
    t_mode = differential & ((r2 < 0) | (r2 > 31))
    h_mode = differential & ~t_mode & ((g2 < 0) | (g2 > 31))
    p_mode = differential & ~t_mode & ~h_mode & ((b2 < 0) | (b2 > 31))
    d_mode = differential & ~t_mode & ~h_mode & ~p_mode
    i_mode = ~differential

    def e5(v):
        return (v << 3) | (v >> 2)

    # base colours of the two sub-blocks (individual / differential)
    base = np.zeros((n, 2, 3), np.int32)
    for ch, (s1, s2) in enumerate(((60, 56), (52, 48), (44, 40))):
        ind1, ind2 = _bits(w, s1, 4) * 17, _bits(w, s2, 4) * 17
        diff1 = e5([rb, gb, bb][ch])
        diff2 = e5(np.clip([r2, g2, b2][ch], 0, 31))
        base[:, 0, ch] = np.where(i_mode, ind1, diff1)
        base[:, 1, ch] = np.where(i_mode, ind2, diff2)
    table = np.stack([_bits(w, 37, 3), _bits(w, 34, 3)], axis=1)

    # T / H paint colours
    def e4(v):
        return v * 17

    t_c1 = np.stack([e4((_bits(w, 59, 2) << 2) | _bits(w, 56, 2)), e4(_bits(w, 52, 4)), e4(_bits(w, 48, 4))], axis=1)
    t_c2 = np.stack([e4(_bits(w, 44, 4)), e4(_bits(w, 40, 4)), e4(_bits(w, 36, 4))], axis=1)
    t_d = TH_DISTANCE[(_bits(w, 34, 2) << 1) | _bits(w, 32, 1)][:, None]
    t_paint = np.stack([t_c1, _clamp255(t_c2 + t_d), t_c2, _clamp255(t_c2 - t_d)], axis=1)  # (N,4,3)
    h1 = [_bits(w, 59, 4), (_bits(w, 56, 3) << 1) | _bits(w, 52, 1), (_bits(w, 51, 1) << 3) | _bits(w, 47, 3)]
    h2 = [_bits(w, 43, 4), _bits(w, 39, 4), _bits(w, 35, 4)]
    h_v1 = (h1[0] << 8) | (h1[1] << 4) | h1[2]
    h_v2 = (h2[0] << 8) | (h2[1] << 4) | h2[2]
    h_d = TH_DISTANCE[(_bits(w, 34, 1) << 2) | (_bits(w, 32, 1) << 1) | (h_v1 >= h_v2).astype(np.int32)][:, None]
    h_c1, h_c2 = np.stack([e4(v) for v in h1], axis=1), np.stack([e4(v) for v in h2], axis=1)
    h_paint = np.stack([_clamp255(h_c1 + h_d), _clamp255(h_c1 - h_d), _clamp255(h_c2 + h_d), _clamp255(h_c2 - h_d)], axis=1)

    # planar
    def e6(v):
        return (v << 2) | (v >> 4)

    def e7(v):
        return (v << 1) | (v >> 6)

    po = [e6(_bits(w, 57, 6)), e7((_bits(w, 56, 1) << 6) | _bits(w, 49, 6)),
          e6((_bits(w, 48, 1) << 5) | (_bits(w, 43, 2) << 3) | _bits(w, 39, 3))]
    ph = [e6((_bits(w, 34, 5) << 1) | _bits(w, 32, 1)), e7(_bits(w, 25, 7)), e6(_bits(w, 19, 6))]
    pv = [e6(_bits(w, 13, 6)), e7(_bits(w, 6, 7)), e6(_bits(w, 0, 6))]

    out = np.zeros((n, 16, 4), np.int32)
    for px in range(16):
        x, y = px & 3, px >> 2
        slot = 4 * x + y
        idx = (_bits(w, 16 + slot, 1) << 1) | _bits(w, slot, 1)
        sub = np.where(flip, y >= 2, x >= 2).astype(np.int32)
        tab = table[np.arange(n), sub]
        mod = np.where(idx & 1, ETC1_MODIFIERS[tab, 1], ETC1_MODIFIERS[tab, 0]) * np.where(idx & 2, -1, 1)
        mod = np.where(~opaque & (idx == 0), 0, mod)  # punch-through, opaque bit 0: index 0 has no offset
        rgb_id = _clamp255(base[np.arange(n), sub] + mod[:, None])
        rgb_t = t_paint[np.arange(n), idx]
        rgb_h = h_paint[np.arange(n), idx]
        rgb_p = np.stack([np.clip((x * (ph[c] - po[c]) + y * (pv[c] - po[c]) + 4 * po[c] + 2) >> 2, 0, 255) for c in range(3)], axis=1)
        rgb = np.where(t_mode[:, None], rgb_t, np.where(h_mode[:, None], rgb_h, np.where(p_mode[:, None], rgb_p, rgb_id)))
        transparent = ~opaque & ~p_mode & (idx == 2)
        out[:, px, :3] = np.where(transparent[:, None], 0, rgb)
        out[:, px, 3] = np.where(transparent, 0, 255)
    return out


def eac(b, off=0, kind=0):
    """(N,16) int32 of an EAC block: kind 0 = 8-bit alpha (0..255), 1 = R11 unsigned (0..2047), 2 = R11 signed (-1023..1023)"""
    w = _be64(b, off)
    base, mult, table = _bits(w, 56, 8), _bits(w, 52, 4), _bits(w, 48, 4)
    out = np.zeros((len(b), 16), np.int32)
    for px in range(16):
        slot = 4 * (px & 3) + (px >> 2)
        mod = EAC_MODIFIERS[table, _bits(w, 45 - 3 * slot, 3)]
        if kind == 0:
            out[:, px] = np.clip(base + mod * mult, 0, 255)
        elif kind == 1:
            out[:, px] = np.clip(base * 8 + 4 + np.where(mult == 0, mod, mod * mult * 8), 0, 2047)
        else:
            sb = np.maximum(np.where(base >= 128, base - 256, base), -127)
            out[:, px] = np.clip(sb * 8 + np.where(mult == 0, mod, mod * mult * 8), -1023, 1023)
    return out


def decode(fmt, packed):
    """packed (N, bytes) uint8 -> the decoded layout of `fmt` (BC7 / BC6H excluded)"""
    fid, bpb, _, _ = FORMATS[fmt]
    b = np.ascontiguousarray(packed, np.uint8).reshape(-1, bpb)
    n = len(b)
    rgba = np.zeros((n, 16, 4), np.int32)
    if fmt == "bc1":
        rgba = bc1_colour(b)[0]
    elif fmt in ("bc2", "bc3"):
        rgba = bc1_colour(b, 8, four_colour_only=True)[0]
        rgba[:, :, 3] = explicit_alpha(b) if fmt == "bc2" else interpolated_alpha(b)
    elif fmt in ("bc4u", "bc4s", "bc5u", "bc5s"):
        sg = fmt.endswith("s")
        rgba[:, :, 0] = interpolated_alpha(b, 0, sg)
        if fmt.startswith("bc5"):
            rgba[:, :, 1] = interpolated_alpha(b, 8, sg)
        rgba[:, :, 3] = 127 if sg else 255
        return rgba.astype(np.int8 if sg else np.uint8)
    elif fmt in ("etc1", "etc2", "etc2rgb"):
        rgba = etc_colour(b)
    elif fmt == "etc2punchthrough":
        rgba = etc_colour(b, punchthrough=True)
    elif fmt == "etc2rgba":
        rgba = etc_colour(b, 8)
        rgba[:, :, 3] = eac(b, 0, 0)
    elif fmt == "eac":
        rgba[:, :, 3] = eac(b, 0, 0)
    elif fmt in ("r11u", "r11s"):
        return eac(b, 0, 1 if fmt == "r11u" else 2).astype(np.int16)
    else:
        raise ValueError("no numpy decoder for %r" % (fmt,))
    return rgba.astype(np.uint8)


def source_values(fmt, source):
    """the source as the encoder reads it, (N,16,4) int32 (R11: (N,16,1)); BC6H: float32"""
    if fmt in ("bc6hu", "bc6hs"):
        return np.ascontiguousarray(source).reshape(-1, 16, 4).astype(np.int16).view(np.float16).astype(np.float32)
    if fmt in ("r11u", "r11s"):
        s = np.ascontiguousarray(source).reshape(-1, 16).astype(np.int16).astype(np.int32)
        s = np.clip(s, 0, 2047) if fmt == "r11u" else np.clip(s, -1023, 1023)
        return s[:, :, None]
    raw = np.ascontiguousarray(source).reshape(-1, 16, 4)
    if fmt in ("bc4s", "bc5s"):
        return np.maximum(raw.view(np.int8).astype(np.int32) if raw.dtype.itemsize == 1 else raw.astype(np.int32), -127)
    return raw.astype(np.int32)


def decoded_values(fmt, decoded):
    if fmt in ("bc6hu", "bc6hs"):
        return np.ascontiguousarray(decoded).reshape(-1, 16, 4).astype(np.int16).view(np.float16).astype(np.float32)
    if fmt in ("r11u", "r11s"):
        return np.asarray(decoded).reshape(-1, 16).astype(np.int32)[:, :, None]
    d = np.asarray(decoded).reshape(-1, 16, 4)
    return d.astype(np.int32)


def block_channel_sse(fmt, decoded, source, valid=None):
    """per-block per-channel squared error.  Integer formats: (N,4) int64, exact.  BC6H: (N,4) float32, each channel summed
    in float32 over texels 0..15, and the (N,) float32 per-block value summed over texel 0..15, channel 0..2 inside.
    valid: optional (N,16) bool of the texels that count (image form)."""
    mask = FORMATS[fmt][2]
    d = decoded_values(fmt, decoded)
    s = source_values(fmt, source)
    n = len(d)
    if valid is None:
        valid = np.ones((n, 16), bool)
    if fmt in ("bc6hu", "bc6hs"):
        per_ch = np.zeros((n, 4), np.float32)
        per_block = np.zeros(n, np.float32)
        for t in range(16):
            for c in range(3):
                diff = d[:, t, c] - s[:, t, c]
                sq = np.where(valid[:, t], diff * diff, np.float32(0)).astype(np.float32)
                per_ch[:, c] = per_ch[:, c] + sq
                per_block = per_block + sq
        return per_ch, per_block
    out = np.zeros((n, 4), np.int64)
    if fmt in ("r11u", "r11s"):
        diff = (d[:, :, 0] - s[:, :, 0]).astype(np.int64)
        out[:, 0] = np.where(valid, diff * diff, 0).sum(axis=1)
        return out, out.sum(axis=1).astype(np.uint32)
    for c in range(4):
        if mask >> c & 1:
            diff = (d[:, :, c] - s[:, :, c]).astype(np.int64)
            out[:, c] = np.where(valid, diff * diff, 0).sum(axis=1)
    return out, out.sum(axis=1).astype(np.uint32)


# The device reduction (decode_kernel.hip): 256 blocks per workgroup, a halving tree in LDS (a[i] += a[i + s], s = 128 ... 1)
# -> one partial per workgroup; a launch covers at most 2^24 blocks; one workgroup of 1024 lanes then sums the partials of a
# launch, lane t taking t, t + 1024, ... in order, and a halving tree over the 1024 lanes; launches add into the totals in order.
WG = 256
TOTAL_WG = 1024
LAUNCH_BLOCKS = 1 << 24


def _tree(v):
    v = v.copy()
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def device_total(per_block_ch, wg=WG, launch=LAUNCH_BLOCKS, total_wg=TOTAL_WG):
    """float64 totals of (N,4) float32 per-block channel sums in the device's order"""
    x = np.asarray(per_block_ch, np.float64)
    total = np.zeros(4, np.float64)
    for first in range(0, len(x), launch):
        part = x[first:first + launch]
        pad = (-len(part)) % wg
        part = np.concatenate([part, np.zeros((pad, 4))]) if pad else part
        partials = _tree(part.reshape(-1, wg, 4).transpose(0, 2, 1))  # (groups, 4)
        pad = (-len(partials)) % total_wg
        partials = np.concatenate([partials, np.zeros((pad, 4))]) if pad else partials
        acc = np.zeros((total_wg, 4), np.float64)
        for row in partials.reshape(-1, total_wg, 4):
            acc = acc + row
        total = total + _tree(acc.T)
    return total


def measure(fmt, decoded, source, valid=None):
    """(totals dict, per-block values) as cvttmi_measure_error reports them"""
    per_ch, per_block = block_channel_sse(fmt, decoded, source, valid)
    n = len(per_ch)
    texels = int(valid.sum()) if valid is not None else 16 * n
    if fmt in ("bc6hu", "bc6hs"):
        return {"sse": [0, 0, 0, 0], "sse_hdr": list(device_total(per_ch)), "texels": texels}, per_block
    return {"sse": [int(v) for v in per_ch.sum(axis=0)], "sse_hdr": [0.0] * 4, "texels": texels}, per_block


def psnr(fmt, sse, texels, mask=0):
    _, _, fmask, peak = FORMATS[fmt]
    mask = mask or fmask
    if peak is None or (mask & ~fmask) or texels == 0:
        return float("nan")
    total = sum(sse[c] for c in range(4) if mask >> c & 1)
    if total == 0:
        return float("inf")
    count = texels * bin(mask).count("1")
    return 10.0 * np.log10(float(peak) * float(peak) * count / float(total))


def image_to_blocks(image, fmt):
    """(H,W,4) image -> (compacted row-major blocks (ceil(H/4)*ceil(W/4),16,4), valid (N,16)); edge texels clamp like
    the tiling kernel (they are not counted)"""
    h, w = image.shape[:2]
    bw, bh = (w + 3) // 4, (h + 3) // 4
    ys = np.minimum(np.arange(bh * 4), h - 1)
    xs = np.minimum(np.arange(bw * 4), w - 1)
    full = image[ys][:, xs]
    blocks = full.reshape(bh, 4, bw, 4, 4).transpose(0, 2, 1, 3, 4).reshape(bh * bw, 16, 4)
    vy = (np.arange(bh * 4) < h).reshape(bh, 4)
    vx = (np.arange(bw * 4) < w).reshape(bw, 4)
    valid = (vy[:, None, :, None] & vx[None, :, None, :]).reshape(bh * bw, 16)
    return blocks, valid
