"""RGBA16F under a mip kernel and in a resize, without a GPU: the names and filter words of the range flags, what the host-only resize
entries refuse and size, the packer's float images, and the anchor of the float32 restatement (tests/hdr_resample_ref.py) against
plain float64 convolution."""
import ctypes
import os

import numpy as np
import pytest

import hdr_resample_ref as ref
import mip_resample_ref as M
from convectionkernels_amd import api, container, packer

E_INVALID = -1
RGBA8, HALF, SNORM = api.PIXELS_RGBA8, api.PIXELS_RGBA16F, api.PIXELS_RGBA8_SNORM
NONNEG, SIGNED = 0x1000, 0x2000
K = api.MIP_KERNELS


# ---- names and words ----

def test_names_and_words():
    assert api.MIP_HDR == {"nonnegative": NONNEG, "signed": SIGNED} == ref.HDR
    assert api.mip_filter_word("box", "lanczos3", "repeat", hdr="nonnegative") == 0x30 | 0x200 | 0x1000
    assert api.mip_filter_word("box", "kaiser", hdr="signed") == 0x40 | 0x2000
    assert api.mip_filter_word("srgb", "kaiser") == 0x41 and api.mip_filter_word("box", None, "clamp", None) == 0
    assert api.resize_filter_word("box", "box", "mirror", hdr="signed") == 0x400 | 0x2000
    assert api.resize_filter_word("lanczos3", hdr="nonnegative") == 0x30 | 0x1000 and api.resize_filter_word() == 0x30
    for call in (lambda: api.mip_filter_word("box", "kaiser", hdr="unsigned"), lambda: api.resize_filter_word(hdr="both"),
                 lambda: api.mip_filter_word("box", "kaiser", hdr=0x1000)):
        with pytest.raises(api.CvttError):
            call()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cvtt_mi355x.h")).read()
    assert "#define CVTTMI_MIP_HDR_NONNEGATIVE 0x1000" in header and "#define CVTTMI_MIP_HDR_SIGNED 0x2000" in header


# ---- the host-only resize entries ----

BAD_WORDS = [(HALF, K["lanczos3"]), (HALF, 0), (HALF, K["kaiser"] | 0x200),                      # RGBA16F without a flag, as before
             (HALF, K["lanczos3"] | NONNEG | SIGNED), (HALF, NONNEG | SIGNED),                   # both flags
             (RGBA8, K["lanczos3"] | NONNEG), (RGBA8, SIGNED), (SNORM, K["kaiser"] | SIGNED),    # a flag with RGBA8 / SNORM
             (HALF, K["lanczos3"] | NONNEG | 1), (HALF, K["lanczos3"] | SIGNED | 2), (HALF, K["mitchell"] | NONNEG | 0x100),
             (RGBA8, K["lanczos3"] | NONNEG | 1), (SNORM, K["lanczos3"] | SIGNED | 2),           # a flag with SRGB / NORMAL / ALPHA_WEIGHTED
             (HALF, K["lanczos3"] | NONNEG | 0x800), (HALF, K["lanczos3"] | 0x800), (RGBA8, K["lanczos3"] | 0x800),   # 0x800 means nothing
             (HALF, K["lanczos3"] | NONNEG | 0x600), (HALF, 0x50 | NONNEG), (HALF, K["lanczos3"] | NONNEG | 0x4000),
             (3, K["lanczos3"] | NONNEG)]


def test_resize_entries_refuse():
    lib = api.load_library()
    need, launches = ctypes.c_size_t(99), ctypes.c_uint32(99)
    for kind, word in BAD_WORDS:
        assert lib.cvttmi_resize_work_bytes(8, 8, 4, 4, kind, word, 1, ctypes.byref(need)) == E_INVALID, (kind, hex(word))
        assert lib.cvttmi_resize_launches(8, 8, 4, 4, kind, word, ctypes.byref(launches)) == E_INVALID, (kind, hex(word))
    assert need.value == 99 and launches.value == 99
    for args in ((0, 8, 4, 4), (8, 8, 4, 65536)):
        assert lib.cvttmi_resize_work_bytes(*args, HALF, K["lanczos3"] | NONNEG, 1, ctypes.byref(need)) == E_INVALID
    with pytest.raises(api.CvttError):
        api.resize_launches(8, 8, 4, 4, "lanczos3", filter="srgb", hdr="signed")


def test_resize_work_bytes_counts_16_byte_entries():
    lib = api.load_library()
    need = ctypes.c_size_t(0)
    for flag in (NONNEG, SIGNED):
        for code in (0,) + tuple(K.values()):
            assert lib.cvttmi_resize_work_bytes(37, 29, 16, 12, HALF, code | flag, 2, ctypes.byref(need)) == 0, hex(code | flag)
        # one launch: the tables alone, exactly those of RGBA8; two launches: the intermediate in entries of 16 bytes
        assert lib.cvttmi_resize_work_bytes(64, 64, 32, 32, HALF, K["lanczos3"] | flag, 3, ctypes.byref(need)) == 0
        assert need.value == 3 * 256 + 256 + 3 * 256 + 256
        assert lib.cvttmi_resize_work_bytes(6, 700, 5, 3, HALF, K["lanczos3"] | flag, 3, ctypes.byref(need)) == 0
        assert need.value == 3 * 256 + 8448 + 3 * 700 * 5 * 16
    assert api.resize_launches(64, 64, 32, 32, "lanczos3", hdr="nonnegative") == 1
    assert api.resize_launches(6, 700, 5, 3, "lanczos3", hdr="signed") == 2
    # the fused-rows limit follows the 16-byte entry: 52 KB hold 52 rows of 64 entries, and no sRGB tables share them
    assert api.resize_launches(64, 128, 64, 64, "box", hdr="signed") == 1      # 16 output rows read 32 + 1 source rows
    assert api.resize_launches(64, 640, 64, 64, "lanczos3", hdr="signed") == 2  # ... 150 + 60 - 1
    assert api.resize_launches(64, 640, 64, 64, "lanczos3") == 2


def test_resize_taps_takes_a_flagged_word():
    lib = api.load_library()
    n = ctypes.c_uint32(0)
    plain_w, plain_f = np.zeros((12, 24), np.int16), np.zeros(12, np.int32)
    assert lib.cvttmi_resize_taps(37, 12, K["lanczos3"], plain_w.ctypes.data, plain_f.ctypes.data, ctypes.byref(n)) == 0
    taps = n.value
    for flag in (NONNEG, SIGNED, NONNEG | 0x200):
        w, f = np.zeros((12, 24), np.int16), np.zeros(12, np.int32)
        assert lib.cvttmi_resize_taps(37, 12, K["lanczos3"] | flag, w.ctypes.data, f.ctypes.data, ctypes.byref(n)) == 0 and n.value == taps
        assert (w == plain_w).all() and (f == plain_f).all()
    assert lib.cvttmi_resize_taps(37, 12, NONNEG, None, None, ctypes.byref(n)) == 0 and n.value == 5
    for word in (K["lanczos3"] | NONNEG | SIGNED, K["lanczos3"] | NONNEG | 1, K["lanczos3"] | SIGNED | 2, K["lanczos3"] | NONNEG | 0x100,
                 K["lanczos3"] | NONNEG | 0x800):
        assert lib.cvttmi_resize_taps(37, 12, word, None, None, ctypes.byref(n)) == E_INVALID, hex(word)


# ---- the packer's float images ----

@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the packer reached the device")
    monkeypatch.setattr(api, "default_context", refuse)
    monkeypatch.setattr(api, "Context", refuse)


def test_packer_loads_float_images(tmp_path):
    rng = np.random.default_rng(3)
    f32 = rng.normal(0.0, 300.0, (5, 7, 4)).astype(np.float32)
    f32[0, 0] = [1e9, -1e9, 65520.0, -65519.9]          # beyond the finite range of a half: clamped, not infinite
    f32[0, 1] = [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 2.0 ** -24]  # ties to even; the smallest subnormal
    np.save(str(tmp_path / "f32.npy"), f32)
    got = packer.load_rgba16f(str(tmp_path / "f32.npy"), "bc6hs")
    assert got.dtype == np.float16 and got.shape == f32.shape and np.isfinite(got).all()
    assert got[0, 0].tolist() == [65504.0, -65504.0, 65504.0, -65504.0]
    assert got[0, 1].view(np.uint16).tolist() == [0x3C00, 0x3C02, 0x0000, 0x0001]
    assert (got == np.clip(f32, -65504, 65504).astype(np.float16)).all()
    f16 = ref.random_finite(rng, (2, 4, 6, 4))
    np.save(str(tmp_path / "f16.npy"), f16.view(np.float16))
    assert (packer.load_layers([str(tmp_path / "f16.npy")], "bc6hu").view(np.uint16) == f16).all()
    np.save(str(tmp_path / "a.npy"), f16[0].view(np.float16))
    np.save(str(tmp_path / "b.npy"), f16[1].view(np.float16).astype(np.float32))
    assert (packer.load_layers([str(tmp_path / "a.npy"), str(tmp_path / "b.npy")], "bc6hu").view(np.uint16) == f16).all()
    assert packer.HALF_FORMATS == {"bc6hu": "nonnegative", "bc6hs": "signed"}


def test_packer_refuses_before_the_device(tmp_path, no_device, capsys):
    out = str(tmp_path / "out.ktx")
    paths = {}
    for name, array in (("u8", np.zeros((8, 12, 4), np.uint8)), ("f64", np.zeros((8, 12, 4), np.float64)), ("rgb", np.zeros((8, 12, 3), np.float16)),
                        ("nan", np.full((8, 12, 4), np.nan, np.float16)), ("inf", np.full((8, 12, 4), np.inf, np.float32)),
                        ("ok", np.ones((8, 12, 4), np.float16)), ("stack", np.ones((2, 8, 8, 4), np.float16))):
        paths[name] = str(tmp_path / (name + ".npy"))
        np.save(paths[name], array)
    (tmp_path / "image.png").write_bytes(b"")
    for fmt in ("bc6hu", "bc6hs"):
        for argv in ([paths["u8"]], ["-mipkernel", "kaiser", paths["u8"]], ["-resize", "4x4", paths["u8"]], ["-pow2", "nearest", paths["u8"]],
                     [paths["f64"]], [paths["rgb"]], [paths["nan"]], [paths["inf"]], [str(tmp_path / "image.png")], [paths["stack"]],
                     ["-array", paths["u8"]], ["-cube", paths["ok"], paths["u8"], paths["ok"], paths["ok"], paths["ok"], paths["ok"]],
                     ["-mipfilter", "srgb", paths["ok"]], ["-mipfilter", "normal", paths["ok"]], ["-alphaweight", paths["ok"]],
                     ["-resize", "4x4", "-resizerule", "srgb", paths["ok"]], ["-maxsize", "4", "-resizerule", "normal", paths["ok"]]):
            assert packer.main(["-format", fmt] + argv + [out]) == 1, (fmt, argv)
            err = capsys.readouterr().err.strip()
            assert fmt in err and "\n" not in err, (fmt, argv, err)
        assert packer.main(["-format", fmt, paths["nan"], out]) == 1 and "non-finite" in capsys.readouterr().err
    assert not (tmp_path / "out.ktx").exists()


def test_packer_passes_the_formats_range(tmp_path, monkeypatch):
    """the range follows the format, goes with a kernel and with every resize, and the image arrives as float16"""
    seen = []

    def resize_file(images, width, height, kernel, rule, wrap, signed=False, ctx=None, hdr=None):
        seen.append(("resize", images.dtype, kernel, rule, hdr))
        return np.zeros(images.shape[:-3] + (height, width, 4), images.dtype)

    def encode_file_mips(image, fmt, options=None, plan=None, ctx=None, mip_filter="box", kernel=None, wrap="clamp", hdr=None):
        seen.append(("mips", image.dtype, image.shape, kernel, hdr))
        return [np.zeros((L.blockCount, 16), np.uint8) for L in api.mip_layout(image.shape[1], image.shape[0], 8, 16)]
    monkeypatch.setattr(packer, "resize_file", resize_file)
    monkeypatch.setattr(packer, "encode_file_mips", encode_file_mips)
    src, out = str(tmp_path / "src.npy"), str(tmp_path / "out.dds")
    np.save(src, np.ones((8, 12, 4), np.float32))
    assert packer.main(["-format", "bc6hu", "-mipkernel", "kaiser", "-dds", src, out]) == 0
    assert seen == [("mips", np.float16, (8, 12, 4), "kaiser", "nonnegative")]
    assert container.read_dds_mips(out)[:3] == ("bc6hu", 12, 8)
    del seen[:]
    assert packer.main(["-format", "bc6hs", "-resize", "20x12", "-mips", src, out]) == 0
    assert seen == [("resize", np.float16, "lanczos3", "box", "signed"), ("mips", np.float16, (12, 20, 4), None, None)]


# ---- the anchor: the float32 restatement against plain float64 convolution ----

def _anchor_images():
    rng = np.random.default_rng(11)
    h, w = 61, 83
    lognormal = np.minimum(np.exp(rng.normal(0.0, 3.0, (h, w, 4))), 65504.0).astype(np.float16)
    gaussian = np.clip(rng.normal(0.0, 50.0, (h, w, 4)), -65504.0, 65504.0).astype(np.float16)
    spikes = np.full((h, w, 4), 0.01, np.float16)
    spikes[::7, ::5] = 65504.0
    return {"log-normal": lognormal.view(np.uint16), "gaussian": gaussian.view(np.uint16), "bit patterns": ref.random_finite(rng, (h, w, 4)),
            "spikes": spikes.view(np.uint16)}


def test_restatement_against_float64():
    """Every product and sum of the rule rounds to float32; the anchor keeps float64 throughout and rounds once, to half, after the
    same clamp.  The two are at most 1 half code apart (asserted), in a share of the values that is printed and stays below 0.5 %:
    a cap chosen so that the rule alone stays well inside it."""
    images = _anchor_images()
    apart = total = 0
    for kernel in api.MIP_KERNELS:
        for flag in (NONNEG, SIGNED):
            for name, img in images.items():
                word = api.MIP_KERNELS[kernel] | flag
                got, want = ref.downsample(img, word), ref.float64_level(img, word)
                d = ref.code_distance(got, want)
                assert got.shape == (30, 41, 4) and d.max() <= 1, (kernel, hex(flag), name, int(d.max()))
                apart += int((d != 0).sum())
                total += d.size
    share = apart / total
    print("float32 restatement against float64: %d of %d values one half code apart (%.4f %%)" % (apart, total, 100.0 * share))
    assert share < 0.005
    # the same through the resize tables, one ratio down and one up
    img = images["log-normal"]
    for size in ((31, 17), (120, 70)):
        d = ref.code_distance(ref.resize(img, *size, "lanczos3", "nonnegative"), ref.float64_resize(img, *size, "lanczos3", "nonnegative"))
        assert d.max() <= 1 and (d != 0).mean() < 0.005


def test_restatement_properties():
    """what the header derives from the rule: at exactly half the resize is the mip level; the same size is the image; the planted
    footprints clamp; under NONNEGATIVE nothing is negative and no -0 comes out; the mip tables are the entry point's"""
    img, spots = ref.planted_image("lanczos3", 40, 30)
    assert len(spots) == 2
    for name, flag in ref.HDR.items():
        level = ref.downsample(img, api.MIP_KERNELS["lanczos3"] | flag)
        assert (ref.resize(img, 20, 15, "lanczos3", name) == level).all()
        (x0, y0, _), (x1, y1, _) = spots
        assert level[y0, x0].tolist() == [0x7BFF] * 4 and level[y1, x1].tolist() == [0xFBFF if flag == SIGNED else 0] * 4
        if flag == NONNEG:
            assert (level < 0x8000).all()
    clean = np.where(img == 0x8000, 0, img)
    assert (ref.resize(clean, 40, 30, "mitchell", "signed") == clean).all()
    assert (ref.resize(clean & 0x7FFF, 40, 30, "box", "nonnegative") == clean & 0x7FFF).all()
    for kernel in api.MIP_KERNELS:
        assert (api.mip_kernel_taps(kernel) == M.taps(kernel)).all()
