"""The mip kernels wider than 2x2 without a GPU: the library's tap tables against the numpy restatement
(tests/mip_resample_ref.py), the generator and the known answers; the int32 bounds the rule rests on; the restatement against
plain float64 arithmetic; the wrap modes; what the kernels are for (less aliasing than the box); names and packer refusals."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest

import mip_filter_ref
import mip_resample_ref as ref
from convectionkernels_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tables as the rule of the header gives them (evaluated in float64).  The request for these kernels printed the Kaiser
# table with central taps 7261, 7261 (7260 before a residual of 2 is split) and sum |w| = 22914.  That table sums to 16386,
# against the rule's own "every table sums to 16384": 16384 x the central float64 weight is 7259.37, so the rule gives 7259,
# the residual is indeed 2, and the taps are 7260, 7260 with sum |w| = 22912.  The other ten taps are as printed.  The rule is
# kept, since everything else (self-reproduction, the bounds) rests on the sum.
KNOWN = {
    "triangle": ([2048, 6144, 6144, 2048], 16384),
    "mitchell": ([-121, -192, 2098, 6407, 6407, 2098, -192, -121], 17636),
    "lanczos3": ([60, 247, -557, -1092, 2220, 7314, 7314, 2220, -1092, -557, 247, 60], 22980),
    "kaiser": ([103, 266, -556, -1076, 2195, 7260, 7260, 2195, -1076, -556, 266, 103], 22912),
}
RULES = {"box": ref.BOX, "srgb": ref.SRGB, "normal": ref.NORMAL}


def _generator():
    spec = importlib.util.spec_from_file_location("gen_mip_kernels", os.path.join(ROOT, "tools", "gen_mip_kernels.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _word(kernel, rule="box", wrap="clamp"):
    return ref.KERNELS[kernel] | RULES[rule] | ref.WRAPS[wrap]


# ---- tap tables ----

@pytest.mark.parametrize("kernel", sorted(KNOWN))
def test_library_taps_are_the_restatement_and_the_known_answers(kernel):
    got = api.mip_kernel_taps(kernel)
    want, abs_sum = KNOWN[kernel]
    assert got.dtype == np.int16 and got.tolist() == want == ref.taps(kernel).tolist()
    assert int(np.abs(got.astype(np.int64)).sum()) == abs_sum
    # symmetric, sums to one, each tap within 1 of 16384 x its float64 weight
    assert got.tolist() == got.tolist()[::-1] and int(got.sum()) == 16384
    assert np.abs(got - 16384.0 * ref.float_taps(kernel)).max() <= 1.0
    assert len(got) == 4 * ref.RADIUS[kernel]


def test_kaiser_centre_before_the_split():
    before = ref.taps("kaiser", split=False)
    assert before[5:7].tolist() == [7259, 7259] and 16384 - int(before.sum()) == 2
    assert abs(16384.0 * ref.float_taps("kaiser")[5] - 7259.374) < 1e-3


def test_taps_entry_point_refuses():
    lib = api.load_library()
    taps, count = np.full(12, 77, np.int16), ctypes.c_uint32(99)
    for word in (0, 1, 0x50, 0xF0, 0x200, 0x100):
        assert lib.cvttmi_mip_kernel_taps(word, taps.ctypes.data, ctypes.byref(count)) == -1, hex(word)
    assert lib.cvttmi_mip_kernel_taps(0x30, None, ctypes.byref(count)) == -1
    assert lib.cvttmi_mip_kernel_taps(0x30, taps.ctypes.data, None) == -1
    assert (taps == 77).all() and count.value == 99
    # the other fields of the word do not matter to the table
    assert lib.cvttmi_mip_kernel_taps(0x10 | 0x400 | 1, taps.ctypes.data, ctypes.byref(count)) == 0
    assert count.value == 4 and taps.tolist() == KNOWN["triangle"][0] + [0] * 8
    assert "cvttmi_mip_kernel_taps" in api.exported_symbols()
    with pytest.raises(api.CvttError):
        api.mip_kernel_taps("box")


def test_generator_renders_the_committed_header():
    m = _generator()
    for target, text in m.render().items():
        assert open(os.path.join(ROOT, target)).read() == text, target
    assert {k: v for k, v in m.build().items()} == {k: v[0] for k, v in KNOWN.items()}


# ---- overflow and self-reproduction ----

@pytest.mark.parametrize("kernel", sorted(KNOWN))
def test_int32_bounds_hold_for_the_committed_tables(kernel):
    w = api.mip_kernel_taps(kernel).astype(np.int64)
    total, pos, neg = int(np.abs(w).sum()), int(w[w > 0].sum()), -int(w[w < 0].sum())
    assert total <= 22980
    # plain and NORMAL: |v| <= 255
    h = total * 255
    hp = (h + 512) >> 10
    assert hp <= 5723 and hp < 1 << 15 and total * hp + (1 << 17) < 1 << 31 and (total * hp + 128) >> 8 < 1 << 20
    # sRGB: 0 <= v <= 65535
    assert total * 65535 <= 1.51e9 and total * 65535 + (1 << 13) < 1 << 31
    hi, lo = (pos * 65535 + (1 << 13)) >> 14, -((-neg * 65535 + (1 << 13)) >> 14)
    assert pos * hi + neg * lo <= 1.6e9 and pos * hi + neg * lo + (1 << 11) < 1 << 31
    assert _generator().bounds(w.tolist())["s_srgb"] == pos * hi + neg * lo


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (3, 5), (16, 16)])
@pytest.mark.parametrize("kernel", sorted(KNOWN))
def test_a_constant_image_reproduces_itself(kernel, shape):
    h, w = shape
    for rule in RULES:
        for wrap in ref.WRAPS:
            for dtype, values in ((np.uint8, (0, 1, 127, 128, 254, 255)), (np.int8, (-128, -127, -1, 0, 1, 127))):
                if dtype == np.int8 and rule == "srgb":
                    continue
                for v in values:
                    img = np.empty((h, w, 4), dtype)
                    img[...] = (v, values[2], values[-1], v)
                    if rule == "normal":
                        # a constant vector comes back normalised, not as itself: one axis at full length does
                        img[...] = (128, 128, 255, v) if dtype == np.uint8 else (0, 0, 127, v)
                    for level in ref.chain(img, _word(kernel, rule, wrap)):
                        assert (level == img[0, 0]).all(), (rule, wrap, v)


# ---- float64 agreement ----

@functools.lru_cache(maxsize=None)
def _random_image(seed=64):
    img = np.random.default_rng(seed).integers(0, 256, (64, 64, 4), dtype=np.uint8)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("rule", ["box", "srgb"])
@pytest.mark.parametrize("kernel", sorted(KNOWN))
def test_restatement_against_float64(kernel, rule):
    """at most one code apart everywhere: tap quantisation moves a result by at most 0.19 code over the two passes, the Q4
    intermediate by 0.05, the last rounding by 0.5.  The share of texels that differ at all is printed, not asserted."""
    for wrap in ref.WRAPS:
        word = _word(kernel, rule, wrap)
        got = ref.downsample(_random_image(), word).astype(np.int64)
        want = ref.float64_level(_random_image(), word)
        diff = np.abs(got - want)
        print("%s %s %s: max difference %d, differing %.3f %%" % (kernel, rule, wrap, diff.max(), 100.0 * (diff != 0).mean()))
        assert diff.max() <= 1, (kernel, rule, wrap)


# ---- worst-case footprints ----

def _python_int_texel(img, taps, x, y, c, srgb=False):
    """the rule in Python integers (no width at all), clamped coordinates"""
    n, (h, w) = len(taps), img.shape[:2]
    table = [int(v) for v in mip_filter_ref.T]
    hs = []
    for j in range(n):
        r = min(max(2 * y + 1 - n // 2 + j, 0), h - 1)
        acc = 0
        for k in range(n):
            v = int(img[r, min(max(2 * x + 1 - n // 2 + k, 0), w - 1), c])
            acc += int(taps[k]) * (table[v] if srgb else v)
        hs.append((acc + (1 << 13)) >> 14 if srgb else (acc + 512) >> 10)
    s = sum(int(taps[j]) * hs[j] for j in range(n))
    if srgb:
        return int(mip_filter_ref.encode(min(max((s + (1 << 11)) >> 12, 0), 4 * 65535))), max(abs(v) for v in hs), abs(s)
    return min(max((s + (1 << 17)) >> 18, 0), 255), max(abs(v) for v in hs), abs(s)


@pytest.mark.parametrize("kernel", sorted(KNOWN))
def test_worst_case_footprints_clamp_and_fit_int32(kernel):
    img, spots = ref.planted_image(kernel, 72, 40)
    assert len(spots) == 3
    zero, spots = spots[2], spots[:2]
    taps = ref.taps(kernel)
    for rule in ("box", "srgb"):
        level = ref.downsample(img, _word(kernel, rule))  # (asserts that every intermediate fits int32)
        for x, y, want in spots:
            assert level[y, x].tolist() == [want] * 4, (rule, x, y)
            for c in range(4):
                got, hmax, smax = _python_int_texel(img, taps, x, y, c, srgb=rule == "srgb" and c < 3)
                assert got == want and smax < 1 << 31 and hmax < (1 << 31 if rule == "srgb" else 1 << 15)
    if kernel == "lanczos3":  # the bounds of the header are reached, not merely respected
        _, hmax, smax = _python_int_texel(img, taps, spots[0][0], spots[0][1], 0, srgb=True)
        assert hmax == (19682 * 65535 + 8192) >> 14 and 1.55e9 < smax <= 1.6e9
    assert (ref.normal_sums(img, _word(kernel, "normal"))[zero[1], zero[0]] == 0).all()
    assert (ref.downsample(img, _word(kernel, "normal"))[zero[1], zero[0]] == ref.downsample(img, _word(kernel))[zero[1], zero[0]]).all()
    signed, spots = ref.planted_image(kernel, 72, 40, np.int8)
    level = ref.downsample(signed, _word(kernel, "box"))
    assert [level[y, x, 0] for x, y, _ in spots[:2]] == [127, -128]
    assert (ref.normal_sums(signed, _word(kernel, "normal"))[spots[2][1], spots[2][0]] == 0).all()


# ---- wrap ----

@pytest.mark.parametrize("kernel", sorted(KNOWN))
def test_repeat_commutes_with_tiling(kernel):
    img = _random_image(9)[:12, :20]
    for rule in ("box", "srgb"):
        word = _word(kernel, rule, "repeat")
        assert (ref.downsample(np.tile(img, (2, 2, 1)), word) == np.tile(ref.downsample(img, word), (2, 2, 1))).all()


@pytest.mark.parametrize("kernel", sorted(KNOWN))
def test_wrap_modes_differ_on_a_ramp(kernel):
    ramp = np.empty((8, 32, 4), np.uint8)
    ramp[...] = (np.arange(32) * 8)[None, :, None]
    levels = {wrap: ref.downsample(ramp, _word(kernel, "box", wrap)) for wrap in ref.WRAPS}
    assert (levels["clamp"] != levels["repeat"]).any() and (levels["mirror"] != levels["repeat"]).any()
    # away from the edges the wrap mode changes nothing
    edge = ref.RADIUS[kernel]
    assert (levels["clamp"][:, edge:-edge] == levels["repeat"][:, edge:-edge]).all()
    assert (levels["clamp"][:, edge:-edge] == levels["mirror"][:, edge:-edge]).all()


def test_mirror_on_an_image_narrower_than_the_footprint():
    def mirror(i, n):  # by hand: walk from 0, turning round at either edge with the edge texel repeated once
        pos, step = 0, 1
        for _ in range(abs(i)) if i >= 0 else range(abs(i) - 1):
            if not 0 <= pos + step < n:
                step = -step
            else:
                pos += step
        return pos
    assert [mirror(i, 3) for i in range(-7, 9)] == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2]
    assert [mirror(i, 3) for i in (-1, 3)] == [0, 2]
    for n in (1, 2, 3, 5):
        idx = np.arange(-14, 15)
        assert ref.wrap_index(idx, n, "mirror").tolist() == [mirror(int(i), n) for i in idx], n
    img = _random_image(3)[:3, :3]
    taps = ref.taps("lanczos3")
    level = ref.downsample(img, _word("lanczos3", "box", "mirror"))
    assert level.shape == (1, 1, 4)
    for c in range(4):
        hs = [(sum(int(taps[k]) * int(img[mirror(2 * 0 + 1 - 6 + j, 3), mirror(1 - 6 + k, 3), c]) for k in range(12)) + 512) >> 10
              for j in range(12)]
        s = sum(int(taps[j]) * hs[j] for j in range(12))
        assert level[0, 0, c] == min(max((s + (1 << 17)) >> 18, 0), 255)


# ---- what the kernels are for ----

def test_less_aliasing_than_the_box():
    """a horizontal sinusoid of period 2.5 source texels lies above the destination's Nyquist frequency: what is left of it in
    level 1 is aliasing.  Only the ordering is asserted."""
    x = np.arange(256)
    wave = np.round(127.5 + 100.0 * np.sin(2 * np.pi * x / 2.5)).astype(np.uint8)
    img = np.empty((16, 256, 4), np.uint8)
    img[...] = wave[None, :, None]

    def swing(level):
        row = level[4, 8:-8, 0].astype(np.int64)
        return int(row.max() - row.min())
    box = swing(mip_filter_ref.downsample(img, "box"))
    left = {k: swing(ref.downsample(img, _word(k))) for k in ("lanczos3", "kaiser")}
    print("peak to peak: box %d, %s" % (box, left))
    assert left["lanczos3"] < box and left["kaiser"] < box


# ---- names and packer refusals ----

def test_names_and_packer_refusals(tmp_path, capsys):
    from convectionkernels_amd import packer
    assert api.MIP_KERNELS == ref.KERNELS == {"triangle": 0x10, "mitchell": 0x20, "lanczos3": 0x30, "kaiser": 0x40}
    assert api.MIP_WRAPS == ref.WRAPS == {"clamp": 0, "repeat": 0x200, "mirror": 0x400}
    assert api.MIP_FILTERS == mip_filter_ref.FILTERS  # unchanged
    assert api.mip_filter_word("srgb", "kaiser", "repeat") == 0x241 and api.mip_filter_word("box") == 0
    assert api.mip_filter_word(api.MIP_FILTER_NORMAL, "triangle", "mirror") == 0x412
    for bad in (dict(kernel="cubic"), dict(kernel=0x10), dict(wrap="border"), dict(wrap=None), dict(filter="linear")):
        with pytest.raises(api.CvttError):
            api.mip_filter_word(**dict(dict(filter="box"), **bad))
    src, out = str(tmp_path / "src.npy"), str(tmp_path / "out.ktx")
    np.save(src, np.zeros((4, 4, 4), np.uint8))
    # refused on the command line, before any device work
    assert packer.main(["-format", "bc7", "-mipkernel", "lanczos3", "-alphaweight", src, out]) == 1
    assert packer.main(["-format", "bc6hu", "-mipkernel", "kaiser", src, out]) == 1
    assert packer.main(["-format", "bc6hs", "-mipkernel", "kaiser", src, out]) == 1
    assert packer.main(["-format", "bc7", "-mips", "-wrap", "repeat", src, out]) == 1
    for err in capsys.readouterr().err.strip().split("\n"):
        assert err and "\n" not in err
    assert packer.main(["-format", "bc7", "-mipkernel", "sinc", src, out]) == 2
    assert packer.main(["-format", "bc7", "-mipkernel", "kaiser", "-wrap", "border", src, out]) == 2
    assert packer.main(["-format", "bc7", "-mipfilter", "cubic", src, out]) == 2
    assert not os.path.exists(out)
    capsys.readouterr()
