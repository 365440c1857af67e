"""Header readers for packed blocks (test helper): which encoding a block uses, not what it decodes to.  Plain numpy,
vectorised over (n, 8 | 16) uint8.  Written from the block-format specifications (BPTC / S3TC / ETC2 / EAC bit layouts);
tests/test_mode_census.py holds the readers to texture_decode_ref.py, the decode goldens and hand-packed blocks.

BC7 / BC6H blocks are little-endian bit streams (bit k = bit k & 7 of byte k >> 3); ETC / EAC words are big-endian."""
import numpy as np

import texture_decode_ref as R


def le_bits(b, start, count):
    """bits start .. start + count - 1 of little-endian bit streams, (n,) int64"""
    b = np.ascontiguousarray(b, np.uint8)
    bits = np.unpackbits(b, axis=1, bitorder="little")[:, start:start + count].astype(np.int64)
    return (bits << np.arange(count, dtype=np.int64)).sum(axis=1)


# ---- BC7 ----
BC7_PARTITION_BITS = {0: 4, 1: 6, 2: 6, 3: 6, 7: 6}           # modes with a partition field, right after the mode bits
BC7_PBITS = {0: (77, 6), 1: (80, 2), 3: (94, 4), 6: (63, 2), 7: (94, 4)}  # (first bit, count); mode 1: one per subset


def bc7_mode(b):
    """0..7 = number of zero bits below the lowest set bit of byte 0; 8 for the reserved all-zero mode byte"""
    m = np.asarray(b)[:, 0].astype(np.int64)
    out = np.full(len(m), 8, np.int64)
    for k in range(7, -1, -1):
        out = np.where((m & ((1 << (k + 1)) - 1)) == (1 << k), k, out)
    return out


def bc7_partition(b):
    """partition of modes 0, 1, 2, 3, 7; -1 for the other modes"""
    mode = bc7_mode(b)
    out = np.full(len(mode), -1, np.int64)
    for m, nbits in BC7_PARTITION_BITS.items():
        out = np.where(mode == m, le_bits(b, m + 1, nbits), out)
    return out


def bc7_rotation(b):
    """rotation of modes 4 and 5; -1 elsewhere"""
    mode = bc7_mode(b)
    return np.where(mode == 4, le_bits(b, 5, 2), np.where(mode == 5, le_bits(b, 6, 2), -1))


def bc7_index_selector(b):
    """index selector of mode 4; -1 elsewhere"""
    return np.where(bc7_mode(b) == 4, le_bits(b, 7, 1), -1)


def bc7_pbits(b):
    """(n, 6) int64: the p-bits of each block in stream order, -1 in the positions its mode does not have"""
    mode = bc7_mode(b)
    out = np.full((len(mode), 6), -1, np.int64)
    for m, (first, count) in BC7_PBITS.items():
        sel = mode == m
        for i in range(count):
            out[:, i] = np.where(sel, le_bits(b, first + i, 1), out[:, i])
    return out


def bc7_label(b):
    """one string per block for mismatch messages"""
    mode, part, rot, sel = bc7_mode(b), bc7_partition(b), bc7_rotation(b), bc7_index_selector(b)
    out = []
    for i in range(len(mode)):
        s = "mode %d" % mode[i]
        if part[i] >= 0:
            s += " partition %d" % part[i]
        if rot[i] >= 0:
            s += " rotation %d" % rot[i]
        if sel[i] >= 0:
            s += " index selector %d" % sel[i]
        out.append(s)
    return out


# ---- BC6H ----
BC6H_TWO_SUBSET_IDS = (0, 1, 2, 6, 10, 14, 18, 22, 26, 30)
BC6H_ONE_SUBSET_IDS = (3, 7, 11, 15)
BC6H_MODE_IDS = BC6H_TWO_SUBSET_IDS + BC6H_ONE_SUBSET_IDS


def bc6h_mode_id(b):
    """the mode field as stored: 0 or 1 (2-bit field), else the 5-bit field (2, 3, 6, 7, ... 30, 31; 19, 23, 27, 31 reserved)"""
    low = le_bits(b, 0, 2)
    return np.where(low < 2, low, le_bits(b, 0, 5))


def bc6h_partition(b):
    """bits 77..81 for the ten two-subset mode ids; -1 for the others"""
    two = np.isin(bc6h_mode_id(b), BC6H_TWO_SUBSET_IDS)
    return np.where(two, le_bits(b, 77, 5), -1)


def bc6h_label(b):
    mode, part = bc6h_mode_id(b), bc6h_partition(b)
    return ["mode id %d" % mode[i] + (" partition %d" % part[i] if part[i] >= 0 else "") for i in range(len(mode))]


# ---- ETC1 / ETC2 colour word ----
def etc_modes(bc, off=0, punchthrough=False):
    """boolean masks of the layout of each colour word at byte `off`: individual, differential, T, H, planar, and (punch-through)
    opaque0 = the opaque bit is 0 in a non-planar block"""
    w = R._be64(bc, off)
    diff = R._bits(w, 33, 1) == 1
    differential = np.ones(len(bc), bool) if punchthrough else diff

    def over(s5, s3):
        v = R._bits(w, s5, 5) + np.where(R._bits(w, s3, 3) >= 4, R._bits(w, s3, 3) - 8, R._bits(w, s3, 3))
        return (v < 0) | (v > 31)
    t = differential & over(59, 56)
    h = differential & ~t & over(51, 48)
    p = differential & ~t & ~h & over(43, 40)
    return {"individual": ~differential, "differential": differential & ~t & ~h & ~p, "T": t, "H": h, "planar": p,
            "opaque0": punchthrough & ~diff & ~p}


ETC_LAYOUTS = ("individual", "differential", "T", "H", "planar")


def etc_layout(bc, off=0, punchthrough=False):
    """(n,) index into ETC_LAYOUTS"""
    modes = etc_modes(bc, off, punchthrough)
    out = np.zeros(len(bc), np.int64)
    for i, name in enumerate(ETC_LAYOUTS):
        out = np.where(modes[name], i, out)
    return out


def etc_flip(bc, off=0):
    """the flip bit (bit 32 of the big-endian word): meaningful for the individual and differential layouts"""
    return R._bits(R._be64(bc, off), 32, 1).astype(np.int64)


def etc_opaque(bc, off=0):
    """punch-through blocks: the opaque bit (where the other formats keep the differential bit)"""
    return R._bits(R._be64(bc, off), 33, 1).astype(np.int64)


def etc_tables(bc, off=0):
    """(n, 2) the table codewords of the two half-blocks (individual / differential layouts)"""
    w = R._be64(bc, off)
    return np.stack([R._bits(w, 37, 3), R._bits(w, 34, 3)], axis=1).astype(np.int64)


def etc_th_distance(bc, off=0, punchthrough=False):
    """the distance index of T and H blocks (H: its lowest bit is the order of the two base colours); -1 for other layouts"""
    w = R._be64(bc, off)
    modes = etc_modes(bc, off, punchthrough)
    t_d = (R._bits(w, 34, 2) << 1) | R._bits(w, 32, 1)
    h1 = (R._bits(w, 59, 4) << 8) | (((R._bits(w, 56, 3) << 1) | R._bits(w, 52, 1)) << 4) | ((R._bits(w, 51, 1) << 3) | R._bits(w, 47, 3))
    h2 = (R._bits(w, 43, 4) << 8) | (R._bits(w, 39, 4) << 4) | R._bits(w, 35, 4)
    h_d = (R._bits(w, 34, 1) << 2) | (R._bits(w, 32, 1) << 1) | (h1 >= h2).astype(np.int32)
    return np.where(modes["T"], t_d, np.where(modes["H"], h_d, -1)).astype(np.int64)


def etc_label(bc, off=0, punchthrough=False):
    lay, flip, tab, dist = etc_layout(bc, off, punchthrough), etc_flip(bc, off), etc_tables(bc, off), etc_th_distance(bc, off, punchthrough)
    out = []
    for i in range(len(lay)):
        name = ETC_LAYOUTS[lay[i]]
        if name in ("individual", "differential"):
            out.append("%s flip %d tables (%d, %d)" % (name, flip[i], tab[i, 0], tab[i, 1]))
        elif name in ("T", "H"):
            out.append("%s distance %d" % (name, dist[i]))
        else:
            out.append(name)
    return out


# ---- EAC / R11 ----
def eac_multiplier(bc, off=0):
    return R._bits(R._be64(bc, off), 52, 4).astype(np.int64)


def eac_table(bc, off=0):
    return R._bits(R._be64(bc, off), 48, 4).astype(np.int64)


def eac_label(bc, off=0):
    m, t = eac_multiplier(bc, off), eac_table(bc, off)
    return ["multiplier %d table %d" % (m[i], t[i]) for i in range(len(m))]


# ---- S3TC ----
def bc1_four_colour(bc, off=0):
    """True: c0 > c1, the four-colour order; False: three colours + transparent black"""
    return R._u16(bc, off) > R._u16(bc, off + 2)


def alpha_eight_value(bc, off=0, signed=False):
    """BC3 alpha / BC4 / BC5 halves: True: a0 > a1, eight interpolated values; False: six values + the two terminals"""
    b = np.asarray(bc)
    dt = np.int8 if signed else np.uint8
    return b[:, off].astype(np.uint8).view(dt).astype(np.int64) > b[:, off + 1].astype(np.uint8).view(dt).astype(np.int64)
