"""Parity on every encoding: directed content and plans (tests/content.py, tests/census_cases.py) that make the reference emit
every BC7 mode x partition / rotation / index selector / p-bit, every BC6H mode id and partition, every ETC layout x flip,
every EAC multiplier and table and both S3TC orders; a census (tests/block_fields.py) that proves it did; and the kernels
held to the reference on exactly those blocks.

CPU: the header readers against texture_decode_ref.py and hand-packed blocks; the C restatement against the reference
(oracle/_ref, where built) and against tests/golden/mode_census.npz (the reference's output, committed); the census
conditions on the restatement's output under the golden's RCPPS table, so they do not depend on the host.
GPU: encoders (BC7: single-mode and default plans x three Options x pruned / exhaustive x host / device), decoders and the
fused error measure on the same bytes, and the golden under its own RCPPS table."""
import os

import numpy as np
import pytest

import block_fields as F
import census_cases as C
import texture_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _threads():
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(round(int(quota) / int(period)))))
    except (OSError, ValueError):
        pass
    return min(n, 16)


def _labels(kind, packed):
    if kind == "bc7":
        return F.bc7_label(packed)
    if kind in ("bc6hu", "bc6hs"):
        return F.bc6h_label(packed)
    if kind in ("etc2", "etc1", "etc2punchthrough"):
        return F.etc_label(packed, 0, kind == "etc2punchthrough")
    if kind == "etc2rgba":
        return ["%s; alpha %s" % (c, a) for c, a in zip(F.etc_label(packed, 8), F.eac_label(packed))]
    if kind in ("eac", "r11u", "r11s"):
        return F.eac_label(packed)
    if kind == "bc1":
        return ["four-colour" if f else "three-colour" for f in F.bc1_four_colour(packed)]
    if kind == "bc2":
        return ["explicit alpha"] * len(packed)
    sg = kind.endswith("s")
    halves = (0, 8) if kind.startswith("bc5") else (0,)
    return ["/".join("eight-value" if F.alpha_eight_value(packed[i:i + 1], off, sg)[0] else "six-value" for off in halves)
            for i in range(len(packed))]


def assert_same_blocks(got, exp, kind, what):
    """every block equal; the message names the encoding (mode, partition, layout ...) of the first differing blocks"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.nonzero((got != exp).any(axis=1))[0]
    if bad.size:
        first = bad[:6]
        want, have = _labels(kind, exp[first]), _labels(kind, got[first])
        lines = ["block %d: expected %s, got %s" % (i, w, h) for i, w, h in zip(first, want, have)]
        pytest.fail("%s: %d of %d blocks differ\n  %s" % (what, bad.size, len(exp), "\n  ".join(lines)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLD, "mode_census.npz"))


@pytest.fixture(scope="module")
def oracle_out(oracle_lib, golden):
    """name -> the restatement's output on every directed case, under the golden's RCPPS table (computed once, read-only)"""
    cache = {}

    def get(case):
        if case[0] not in cache:
            out = C.encode_oracle(oracle_lib, case, golden["rcp"], _threads())
            out.setflags(write=False)
            cache[case[0]] = out
        return cache[case[0]]
    return get


# ================================================================ CPU: the header readers

def _pack_le(value):
    return np.frombuffer(int(value).to_bytes(16, "little"), np.uint8).copy()


def test_bc7_readers_on_hand_packed_blocks():
    rng = np.random.Generator(np.random.PCG64(1))
    blocks, want = [], []
    for mode in range(8):
        for trial in range(24):
            v = int.from_bytes(rng.bytes(16), "little")
            v = (v >> (mode + 1) << (mode + 1)) | (1 << mode)  # mode: `mode` zero bits, then a one
            fields = {"mode": mode, "partition": -1, "rotation": -1, "sel": -1, "pbits": [-1] * 6}
            if mode in F.BC7_PARTITION_BITS:
                nbits = F.BC7_PARTITION_BITS[mode]
                part = int(rng.integers(0, 1 << nbits))
                v = (v & ~(((1 << nbits) - 1) << (mode + 1))) | (part << (mode + 1))
                fields["partition"] = part
            if mode in (4, 5):
                rot = trial % 4
                v = (v & ~(3 << (mode + 1))) | (rot << (mode + 1))
                fields["rotation"] = rot
            if mode == 4:
                sel = (trial >> 2) & 1
                v = (v & ~(1 << 7)) | (sel << 7)
                fields["sel"] = sel
            if mode in F.BC7_PBITS:
                first, count = F.BC7_PBITS[mode]
                bits = [int(x) for x in rng.integers(0, 2, count)]
                for i, bit in enumerate(bits):
                    v = (v & ~(1 << (first + i))) | (bit << (first + i))
                fields["pbits"] = bits + [-1] * (6 - count)
            blocks.append(_pack_le(v))
            want.append(fields)
    b = np.stack(blocks)
    assert F.bc7_mode(b).tolist() == [w["mode"] for w in want]
    assert F.bc7_partition(b).tolist() == [w["partition"] for w in want]
    assert F.bc7_rotation(b).tolist() == [w["rotation"] for w in want]
    assert F.bc7_index_selector(b).tolist() == [w["sel"] for w in want]
    assert F.bc7_pbits(b).tolist() == [w["pbits"] for w in want]
    assert F.bc7_mode(np.zeros((1, 16), np.uint8)).tolist() == [8]
    # the field widths add up to 128 bits: mode + partition + rotation / selector + endpoints + p-bits + indices
    # (subsets, colour bits, alpha bits, p-bits, index bits, second index bits) per mode, from the BPTC specification
    spec = {0: (3, 4, 0, 6, 45, 0), 1: (2, 6, 0, 2, 46, 0), 2: (3, 5, 0, 0, 29, 0), 3: (2, 7, 0, 4, 30, 0),
            4: (1, 5, 6, 0, 31, 47), 5: (1, 7, 8, 0, 31, 31), 6: (1, 7, 7, 2, 63, 0), 7: (2, 5, 5, 4, 30, 0)}
    for mode, (subsets, cb, ab, pb, ib, ib2) in spec.items():
        header = mode + 1 + F.BC7_PARTITION_BITS.get(mode, 0) + (2 if mode in (4, 5) else 0) + (1 if mode == 4 else 0)
        endpoints = subsets * 2 * (3 * cb + ab)
        assert header + endpoints + pb + ib + ib2 == 128, mode
        if mode in F.BC7_PBITS:
            assert F.BC7_PBITS[mode] == (header + endpoints, pb), mode


def test_bc7_mode_reader_against_decode_golden():
    """a block whose mode byte is reserved decodes to zero; every other mode of decode.npz is 0..7"""
    g = np.load(os.path.join(GOLD, "decode.npz"))
    mode = F.bc7_mode(g["bc7_in"])
    assert (g["bc7_out"][mode == 8] == 0).all() and (mode[-8:] == 8).all()
    assert set(mode.tolist()) == set(range(9))


def test_bc6h_readers_on_hand_packed_blocks():
    rng = np.random.Generator(np.random.PCG64(2))
    blocks, modes, parts = [], [], []
    for mode in F.BC6H_MODE_IDS + (19, 23, 27, 31):
        for part in range(32):
            v = int.from_bytes(rng.bytes(16), "little")
            width = 2 if mode < 2 else 5
            v = (v >> width << width) | mode
            v = (v & ~(31 << 77)) | (part << 77)
            blocks.append(_pack_le(v))
            modes.append(mode)
            parts.append(part if mode in F.BC6H_TWO_SUBSET_IDS else -1)
    b = np.stack(blocks)
    assert F.bc6h_mode_id(b).tolist() == modes
    assert F.bc6h_partition(b).tolist() == parts
    assert len(F.BC6H_MODE_IDS) == 14 and len(set(F.BC6H_MODE_IDS)) == 14


def _be_word(value):
    return np.frombuffer(int(value).to_bytes(8, "big"), np.uint8).copy()


def test_etc_readers_on_hand_packed_words():
    words, want = [], []
    for flip in range(2):
        for t0 in range(8):
            t1 = (t0 * 3 + flip) % 8
            tail = (t0 << 37) | (t1 << 34) | (flip << 32) | 0x12345678
            # individual: diff bit 0
            words.append((0xA5 << 56) | (0x3C << 48) | (0x7E << 40) | tail)
            want.append(("individual", flip, t0, t1))
            # differential: diff bit 1, base + delta inside 0..31 in every channel
            words.append((((10 << 3) | 3) << 56) | (((20 << 3) | 5) << 48) | (((1 << 3) | 7) << 40) | (1 << 33) | tail)
            want.append(("differential", flip, t0, t1))
    # T: red overflows (base 1, delta -3); H: green overflows (31 + 2); planar: blue overflows (0 - 1)
    for name, hi in (("T", (((1 << 3) | 5) << 56) | (0x55 << 48) | (0x55 << 40)),
                     ("H", (((10 << 3) | 1) << 56) | (((31 << 3) | 2) << 48) | (0x55 << 40)),
                     ("planar", (((10 << 3) | 1) << 56) | (((20 << 3) | 1) << 48) | (((0 << 3) | 7) << 40))):
        words.append(hi | (1 << 33) | 0x0F0F1234)
        want.append((name, None, None, None))
    b = np.stack([_be_word(w) for w in words])
    lay, flip, tab = F.etc_layout(b), F.etc_flip(b), F.etc_tables(b)
    for i, (name, fl, t0, t1) in enumerate(want):
        assert F.ETC_LAYOUTS[lay[i]] == name, i
        if fl is not None:
            assert (flip[i], tab[i, 0], tab[i, 1]) == (fl, t0, t1), i
    # punch-through: bit 33 is the opaque bit, every block is differential-coded
    pt = F.etc_modes(b[:2], punchthrough=True)
    assert pt["differential"].all() and not pt["individual"].any()
    assert F.etc_opaque(b[:2]).tolist() == [0, 1]


def test_etc_and_eac_readers_against_the_numpy_decoder():
    """what the readers say of random words reproduces texture_decode_ref's pixels: the corner pixels of individual /
    differential blocks from (flip, tables), the paint distance of T / H blocks, EAC values from (multiplier, table)"""
    rng = np.random.Generator(np.random.PCG64(3))
    b = rng.integers(0, 256, (4096, 8), dtype=np.uint8)
    w = R._be64(b, 0)
    lay, flip, tab = F.etc_layout(b), F.etc_flip(b), F.etc_tables(b)
    dec = R.etc_colour(b).astype(np.int64)
    sel = lay <= 1
    assert sel.sum() > 500 and (lay == 0).sum() > 100 and (lay == 1).sum() > 100

    def sext3(v):
        return np.where(v >= 4, v - 8, v)
    base = np.zeros((len(b), 2, 3), np.int64)
    for ch, s5 in enumerate((59, 51, 43)):
        five, d3 = R._bits(w, s5, 5), sext3(R._bits(w, s5 - 3, 3))
        second = five + d3
        base[:, 0, ch] = np.where(lay == 0, R._bits(w, s5 + 1, 4) * 17, (five << 3) | (five >> 2))
        base[:, 1, ch] = np.where(lay == 0, R._bits(w, s5 - 3, 4) * 17, (second << 3) | (second >> 2))
    for px, sub in ((0, np.zeros(len(b), np.int64)), (15, np.ones(len(b), np.int64)), (3, 1 - flip), (12, flip)):
        x, y = px & 3, px >> 2
        slot = 4 * x + y
        idx = (R._bits(w, 16 + slot, 1) << 1) | R._bits(w, slot, 1)
        t = tab[np.arange(len(b)), sub]
        mod = np.where(idx & 1, R.ETC1_MODIFIERS[t, 1], R.ETC1_MODIFIERS[t, 0]) * np.where(idx & 2, -1, 1)
        exp = np.clip(base[np.arange(len(b)), sub] + mod[:, None], 0, 255)
        assert (dec[sel, px, :3] == exp[sel]).all(), px
    # T / H: with every selector 1 and then 3 (T: c2 +- d; H: c1 - d is selector 1, c2 - d selector 3, + d selectors 0 and 2)
    dist = F.etc_th_distance(b)
    for layout, (plus, minus) in ((2, (1, 3)), (3, (0, 1))):
        seen = set()

        def with_selector(v):
            c = b.copy()
            c[:, 4:6] = 0xFF if v & 2 else 0
            c[:, 6:8] = 0xFF if v & 1 else 0
            return R.etc_colour(c).astype(np.int64)[:, 0, :3]
        hi, lo = with_selector(plus), with_selector(minus)
        # (H: the distance's lowest bit compares the base colours, which the selectors do not touch; T: bit 32 is not a selector)
        for i in np.nonzero(lay == layout)[0]:
            ok = (hi[i] < 255) & (lo[i] > 0)
            if ok.any():
                assert ((hi[i] - lo[i])[ok] == 2 * R.TH_DISTANCE[dist[i]]).all(), (layout, i)
                seen.add(int(dist[i]))
        assert seen == set(range(8)), layout
    # EAC
    mult, table = F.eac_multiplier(b), F.eac_table(b)
    basev = b[:, 0].astype(np.int64)
    for px in (0, 5, 15):
        slot = 4 * (px & 3) + (px >> 2)
        mod = R.EAC_MODIFIERS[table, R._bits(w, 45 - 3 * slot, 3)]
        assert (R.eac(b, 0, 0)[:, px] == np.clip(basev + mod * mult, 0, 255)).all()
        assert (R.eac(b, 0, 1)[:, px] == np.clip(basev * 8 + 4 + np.where(mult == 0, mod, mod * mult * 8), 0, 2047)).all()
    assert set(mult.tolist()) == set(range(16)) and set(table.tolist()) == set(range(16))


def test_s3tc_readers_against_the_numpy_decoder():
    """three-colour BC1 blocks are the ones whose selector 3 decodes transparent; six-value alpha blocks the ones whose
    selectors 6 and 7 decode to the terminals"""
    rng = np.random.Generator(np.random.PCG64(4))
    b = rng.integers(0, 256, (2048, 8), dtype=np.uint8)
    b[:, 4:] = 0xFF  # every selector 3
    assert ((R.decode("bc1", b)[:, 0, 3] == 0) == ~F.bc1_four_colour(b)).all()
    a = rng.integers(0, 256, (2048, 8), dtype=np.uint8)
    a[:, 2:] = 0xFF  # every selector 7
    a = a[a[:, 0] != a[:, 1]]
    for signed, fmt, high in ((False, "bc4u", 255), (True, "bc4s", 127)):
        a2 = a[(a[:, :2] != 128).all(axis=1) & (a[:, :2] != high).all(axis=1)] if signed else a[(a[:, :2] != 255).all(axis=1)]
        six = ~F.alpha_eight_value(a2, 0, signed)
        assert ((R.decode(fmt, a2)[:, 0, 0] == high) == six).all(), fmt
        assert six.sum() > 100 and (~six).sum() > 100


# ================================================================ CPU: restatement == reference == golden

CASE_GROUPS = (["bc7_" + k for k in ("0", "1", "2", "3", "7a", "7o", "4", "5", "6")] + ["bc6hu", "bc6hs"]
               + list(C.ETC_KINDS + C.EAC_KINDS + C.S3TC_KINDS))


def _group_cases(group):
    if group.startswith("bc7_"):
        return C.bc7_cases(group[4:])
    if group in ("bc6hu", "bc6hs"):
        return C.bc6h_cases(group == "bc6hs")
    return [C.simple_case(group)]


def test_case_groups_cover_every_case():
    assert [c[0] for g in CASE_GROUPS for c in _group_cases(g)] == [c[0] for c in C.all_cases()]


def _reference(ref, case, threads):
    """the reference on one case, BC7 and BC6H on every host thread (the shim's own std::threads)"""
    name, kind, blocks, ob, pb = case
    if kind in ("bc7", "bc6hu", "bc6hs"):
        out, done, _ = ref.encode_mt(kind, blocks, ob, pb, threads=threads, budget_s=600.0, chunk_blocks=8)  # whole chunks only
        assert done == len(blocks)
        return out
    return C.encode_reference(ref, case)


@pytest.mark.parametrize("group", CASE_GROUPS)
def test_oracle_equals_reference(oracle_lib, ref_lib, group):
    """without this the restatement could share a kernel's mistake on exactly the encodings nothing else reaches"""
    rcp = ref_lib.probe_rcp()
    for case in _group_cases(group):
        exp = _reference(ref_lib, case, _threads())
        got = C.encode_oracle(oracle_lib, case, rcp, _threads())
        assert_same_blocks(got, exp, case[1], "restatement vs reference, " + case[0])


@pytest.mark.parametrize("group", CASE_GROUPS)
def test_oracle_equals_golden(oracle_out, golden, group):
    """the directed cases stay pinned to the reference where oracle/_ref is absent"""
    for case in _group_cases(group):
        name, kind, _, ob, pb = case
        assert (golden["opt_" + name] == ob).all(), name
        if pb is not None:
            assert (golden["plan_" + name] == pb).all(), name
        assert_same_blocks(oracle_out(case), golden["out_" + name], kind, "restatement vs golden, " + name)


def test_golden_lists_every_case(golden):
    assert list(golden["names"]) == [c[0] for c in C.all_cases()]


# ================================================================ CPU: the census conditions (on expected bytes only)

def _bc7_union(oracle_out, key, plan):
    outs = [oracle_out(c) for c in C.bc7_cases(key) if ("_%s_" % plan) in c[0]]
    return np.concatenate(outs)


@pytest.mark.parametrize("key,mode,partitions", [("0", 0, 16), ("1", 1, 64), ("2", 2, 64), ("3", 3, 64), ("7a", 7, 64), ("7o", 7, 64)])
def test_census_bc7_every_partition(oracle_out, key, mode, partitions):
    """under its single-mode plan every block of a shaped set takes the steered mode, every partition of the mode occurs --
    mode 7 from alpha content and from opaque content separately -- and nearly every block takes the partition it was
    shaped after; both values of every p-bit position occur"""
    for case in C.bc7_cases(key):
        if "_single_" not in case[0]:
            continue
        out = oracle_out(case)
        assert (F.bc7_mode(out) == mode).all(), case[0]
        part = F.bc7_partition(out)
        assert set(part.tolist()) == set(range(partitions)), case[0]
        shaped = np.arange(len(out)) // 8
        # the shaped partition wins unless noise or quantisation makes a neighbouring shape as good: 4 blocks in 5 at least
        assert (part == shaped).sum() >= len(out) * 4 // 5, case[0]
        pbits = F.bc7_pbits(out)
        if mode in F.BC7_PBITS:
            for i in range(F.BC7_PBITS[mode][1]):
                assert set(pbits[:, i].tolist()) == {0, 1}, (case[0], i)
        else:
            assert (pbits == -1).all()
    if key == "7a":
        assert (C.bc7_sets()[key][1][:, :, 3] != 255).any(axis=1).all()
    if key == "7o":
        assert (C.bc7_sets()[key][1][:, :, 3] == 255).all()


def test_census_bc7_default_plan_reaches_the_steered_modes(oracle_out):
    """the default plan lets the other modes compete: modes 0, 1 and 7 (alpha content) still reach every partition"""
    for key, mode, partitions in (("0", 0, 16), ("1", 1, 64), ("7a", 7, 64)):
        out = _bc7_union(oracle_out, key, "default")
        assert set(F.bc7_partition(out[F.bc7_mode(out) == mode]).tolist()) == set(range(partitions)), key


def test_census_bc7_dual_plane_and_mode6(oracle_out):
    out4 = _bc7_union(oracle_out, "4", "single")
    m4 = F.bc7_mode(out4) == 4
    assert set(zip(F.bc7_rotation(out4[m4]).tolist(), F.bc7_index_selector(out4[m4]).tolist())) == {(r, s) for r in range(4) for s in range(2)}
    out5 = _bc7_union(oracle_out, "5", "single")
    assert set(F.bc7_rotation(out5[F.bc7_mode(out5) == 5]).tolist()) == {0, 1, 2, 3}
    out6 = _bc7_union(oracle_out, "6", "single")
    m6 = F.bc7_mode(out6) == 6
    assert m6.sum() >= 64
    assert set(F.bc7_pbits(out6[m6])[:, 0].tolist()) == {0, 1} and set(F.bc7_pbits(out6[m6])[:, 1].tolist()) == {0, 1}
    # under the default plan the three compete on the same content and all of them win somewhere
    mixed = F.bc7_mode(_bc7_union(oracle_out, "4", "default"))
    assert {4, 5, 6} <= set(mixed.tolist())


# (mode id, partition) pairs the directed BC6H content does not reach, union over the three option sets.  A pair that appears
# here is device code no test compares with the reference; the sets may only shrink.
BC6H_MISSING = {
    False: {(6, 0)},
    True: {(6, 19), (6, 31)},
}
BC6H_PAIR_FLOOR = {False: 300, True: 280}


@pytest.mark.parametrize("signed", [False, True])
def test_census_bc6h(oracle_out, signed):
    pairs, ids = set(), set()
    for case in C.bc6h_cases(signed):
        out = oracle_out(case)
        mode, part = F.bc6h_mode_id(out), F.bc6h_partition(out)
        ids |= set(mode.tolist())
        pairs |= set(zip(mode[part >= 0].tolist(), part[part >= 0].tolist()))
    assert ids == set(F.BC6H_MODE_IDS)
    assert {p for _, p in pairs} == set(range(32))
    every = {(m, p) for m in F.BC6H_TWO_SUBSET_IDS for p in range(32)}
    assert len(every) == 320 and pairs <= every
    assert len(pairs) >= BC6H_PAIR_FLOOR[signed]
    assert every - pairs == BC6H_MISSING[signed]
    # each delta-coded mode whose budget binds in one channel only (ids 6, 10, 22, 26) in most partitions
    for m in (6, 10, 22, 26):
        assert len({p for mm, p in pairs if mm == m}) >= 24, m


@pytest.mark.parametrize("kind", C.ETC_KINDS)
def test_census_etc(oracle_out, kind):
    """every layout the format has x both flips.  ETC2 RGB / RGBA / punch-through never emit the individual layout: the
    reference hands its ETC2 path to the ETC1 search with the differential-only switch set (CompressETC2Block calls
    CompressETC1BlockInternal with punchthrough = true for every ETC2 format, which starts its loop over the two codings at
    the differential one), so no content can make it win there; half-blocks with far-apart bases and four luma levels each
    -- where individual beats differential and H in ETC1 -- were tried and gave T / H.  ETC1 emits it, and is required to."""
    _assert_etc_census(oracle_out(C.simple_case(kind)), kind)


def _assert_etc_census(out, kind):
    """the conditions of test_census_etc on one case's expected bytes"""
    off = 8 if kind == "etc2rgba" else 0
    pt = kind == "etc2punchthrough"
    lay, flip = F.etc_layout(out, off, pt), F.etc_flip(out, off)
    layouts = {"etc1": ("individual", "differential"), "etc2": ("differential", "T", "H", "planar"),
               "etc2rgba": ("differential", "T", "H", "planar"), "etc2punchthrough": ("differential", "T", "H", "planar")}[kind]
    got = {(F.ETC_LAYOUTS[l], f) for l, f in zip(lay.tolist(), flip.tolist())}
    assert got == {(name, f) for name in layouts for f in range(2)}
    coded = lay <= 1
    assert len(set(map(tuple, F.etc_tables(out, off)[coded].tolist()))) >= 54
    if kind != "etc1":
        dist = F.etc_th_distance(out, off, pt)
        assert set(dist[lay == 2].tolist()) == set(range(8)) and set(dist[lay == 3].tolist()) == set(range(8))
    if pt:
        assert set(F.etc_opaque(out).tolist()) == {0, 1}
        assert F.etc_modes(out, 0, True)["opaque0"].sum() >= 16


ETC_OPTION_CASES = [c[0] for c in C.etc_option_cases()]


def _etc_option_case(name):
    return next(c for c in C.etc_option_cases() if c[0] == name)


@pytest.mark.parametrize("name", ETC_OPTION_CASES)
def test_etc_option_case_oracle_equals_reference(oracle_lib, ref_lib, name):
    """the FAKE instantiations, the uniform and the re-weighted metric on directed content: the restatement stays the reference"""
    case = _etc_option_case(name)
    assert_same_blocks(C.encode_oracle(oracle_lib, case, None, _threads()), C.encode_reference(ref_lib, case), case[1],
                       "restatement vs reference, " + name)


@pytest.mark.parametrize("name", ETC_OPTION_CASES)
def test_census_etc_option_case(oracle_out, name):
    """every ETC format under every option set of census_cases.etc_options still emits every layout it can x both flips, every
    T / H distance and, punch-through, both opacities: the conditions of test_census_etc, unchanged.  The fake-BT.709 metric
    with weights below it starves the T mode of its larger distances on the default content (the reference scores the line
    paints with the weighted metric against luma / chroma: only near-black blocks survive); content.fake709_t_blocks puts
    them back for these cases."""
    case = _etc_option_case(name)
    _assert_etc_census(oracle_out(case), case[1])


@pytest.mark.parametrize("kind", C.EAC_KINDS)
def test_census_eac(oracle_out, kind):
    """every multiplier and every table.  8-bit EAC never stores multiplier 0: the reference clamps its candidate multipliers
    to 1..15 there (CompressETC2AlphaBlockInternal), and only the 11-bit path, whose multiplier 0 means steps of 1 / 8, goes
    below"""
    out = oracle_out(C.simple_case(kind))
    mult, table = F.eac_multiplier(out), F.eac_table(out)
    assert set(table.tolist()) == set(range(16))
    assert set(mult.tolist()) == (set(range(16)) if kind in ("r11u", "r11s") else set(range(1, 16)))


def test_census_s3tc(oracle_out):
    out = oracle_out(C.simple_case("bc1"))
    assert set(F.bc1_four_colour(out).tolist()) == {False, True}
    for kind in ("bc3", "bc4u", "bc4s", "bc5u", "bc5s"):
        out = oracle_out(C.simple_case(kind))
        for off in ((0, 8) if kind.startswith("bc5") else (0,)):
            order = F.alpha_eight_value(out, off, kind.endswith("s"))
            assert min(order.sum(), (~order).sum()) >= 32, (kind, off)


# ================================================================ GPU

class _Expect:
    """what the kernels must produce: the reference where oracle/_ref travelled, else the restatement, under the box's RCPPS table"""

    def __init__(self, oracle_lib):
        from oracle import pyref
        self.orc = oracle_lib
        self.ref = pyref.RefLib() if pyref.RefLib.available() else None
        self.kind = "reference" if self.ref else "restatement"
        self.rcp = (self.ref or self.orc).probe_rcp()
        self.threads = _threads()
        self.cache = {}

    def __call__(self, case):
        if case[0] not in self.cache:
            out = _reference(self.ref, case, self.threads) if self.ref else C.encode_oracle(self.orc, case, self.rcp, self.threads)
            out.setflags(write=False)
            self.cache[case[0]] = out
        return self.cache[case[0]]


@pytest.fixture(scope="module")
def expect(oracle_lib):
    return _Expect(oracle_lib)


def _gpu_both_paths(gpu_ctx, case, exp, what):
    import torch
    _, kind, blocks, _, _ = case
    assert_same_blocks(C.encode_gpu(gpu_ctx, case), exp, kind, "%s, host path" % what)
    dev = torch.from_numpy(np.ascontiguousarray(C.source_for(kind, blocks))).cuda()
    assert_same_blocks(C.encode_gpu(gpu_ctx, case, dev).cpu().numpy(), exp, kind, "%s, device tensor" % what)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["0", "1", "2", "3", "7a", "7o", "4", "5", "6"])
def test_gpu_bc7_directed(gpu_ctx, expect, key):
    gpu_ctx.set_rcp_table(expect.rcp)
    try:
        for case in C.bc7_cases(key):
            exp = expect(case)
            for exhaustive in (False, True):
                gpu_ctx.set_exhaustive(exhaustive)
                _gpu_both_paths(gpu_ctx, case, exp, "%s vs %s, %s" % (case[0], expect.kind, "exhaustive" if exhaustive else "pruned"))
    finally:
        gpu_ctx.set_exhaustive(False)


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [False, True])
def test_gpu_bc6h_directed(gpu_ctx, expect, signed):
    gpu_ctx.set_rcp_table(expect.rcp)
    for case in C.bc6h_cases(signed):
        exp = expect(case)
        _gpu_both_paths(gpu_ctx, case, exp, "%s vs %s" % (case[0], expect.kind))
        for n in (8, 72):  # ragged sizes: one group, and nine (groups are independent, so the expected bytes are a prefix)
            got = C.encode_gpu(gpu_ctx, case, case[2][:n])
            assert_same_blocks(got, exp[:n], case[1], "%s, first %d blocks" % (case[0], n))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", C.ETC_KINDS + C.EAC_KINDS + C.S3TC_KINDS)
def test_gpu_ldr_directed(gpu_ctx, expect, kind):
    gpu_ctx.set_rcp_table(expect.rcp)
    case = C.simple_case(kind)
    _gpu_both_paths(gpu_ctx, case, expect(case), "%s vs %s" % (case[0], expect.kind))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ETC_OPTION_CASES)
def test_gpu_etc_option_case(gpu_ctx, expect, name):
    """the FAKE instantiations of the ETC kernel (table and accurate rounding), the uniform and the re-weighted metric on content
    that reaches every mode under them: host array and device tensor, the whole set, one group and nine"""
    gpu_ctx.set_rcp_table(expect.rcp)
    case = _etc_option_case(name)
    exp = expect(case)
    _gpu_both_paths(gpu_ctx, case, exp, "%s vs %s" % (name, expect.kind))
    for n in (8, 72):
        _gpu_both_paths(gpu_ctx, case[:2] + (case[2][:n],) + case[3:], exp[:n], "%s, first %d blocks" % (name, n))


@pytest.mark.gpu
@pytest.mark.parametrize("group", CASE_GROUPS)
def test_gpu_equals_golden(gpu_ctx, golden, group):
    gpu_ctx.set_rcp_table(golden["rcp"])
    for case in _group_cases(group):
        assert_same_blocks(C.encode_gpu(gpu_ctx, case), golden["out_" + case[0]], case[1], "kernel vs golden, " + case[0])


def _reference_decoded(gpu_ctx, kind, packed):
    """BC7 / BC6H decoded by the reference where oracle/_ref is present.  Where it is not, the kernels' own decoder stands in:
    the decode comparison then says nothing, and the measure is still held to the restatement's arithmetic"""
    from oracle import pyref
    if pyref.RefLib.available():
        ref = pyref.RefLib()
        return ref.decode_bc7(packed) if kind == "bc7" else ref.decode_bc6h(packed, kind == "bc6hs")
    return gpu_ctx.decode(kind, packed)


@pytest.mark.gpu
@pytest.mark.parametrize("group", CASE_GROUPS)
def test_gpu_decoders_and_measure_on_every_encoding(gpu_ctx, golden, group):
    """the expected bytes of every directed case -- so every (mode, partition), layout and table -- through the decoders and
    the fused measure: BC7 / BC6H against the reference's decoders where present, the other formats against the numpy
    restatement; per-block error against the restatement of the measure"""
    import torch
    for case in _group_cases(group):
        name, kind, blocks, _, _ = case
        packed = np.ascontiguousarray(golden["out_" + name])
        source = np.ascontiguousarray(C.source_for(kind, blocks))
        if kind in ("bc7", "bc6hu", "bc6hs"):
            exp_dec = _reference_decoded(gpu_ctx, kind, packed)
        else:
            exp_dec = R.decode(kind, packed)
        host = gpu_ctx.decode(kind, packed)
        dev = gpu_ctx.decode(kind, torch.from_numpy(packed).cuda()).cpu().numpy()
        for got, path in ((host, "host"), (dev, "device")):
            bad = np.nonzero((got.reshape(len(packed), -1) != exp_dec.reshape(len(packed), -1)).any(axis=1))[0]
            assert bad.size == 0, "decode %s (%s): %d blocks differ, first: %s" % (
                name, path, bad.size, list(zip(bad[:6].tolist(), _labels(kind, packed[bad[:6]]))))
        exp, exp_pb = R.measure(kind, exp_dec, source)
        rep = gpu_ctx.measure_error(kind, source, packed, per_block=True)
        if kind in ("bc6hu", "bc6hs"):
            same = (rep.per_block.view(np.uint32) == exp_pb.view(np.uint32)) | (np.isnan(rep.per_block) & np.isnan(exp_pb))
            assert np.array_equal(np.array(rep.totals.sseHdr), np.array(exp["sse_hdr"]), equal_nan=True), name
        else:
            same = rep.per_block.astype(np.uint32) == exp_pb
            assert list(rep.totals.sse) == exp["sse"], name
        bad = np.nonzero(~same)[0]
        assert bad.size == 0, "measure %s: %d blocks differ, first: %s" % (
            name, bad.size, list(zip(bad[:6].tolist(), _labels(kind, packed[bad[:6]]))))
