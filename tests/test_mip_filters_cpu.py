"""The mip filters without a GPU: the library's sRGB tables against the numpy restatement (tests/mip_filter_ref.py) and the
generator, the properties the rules rest on, the restatement against plain float64 arithmetic, a few quads by hand, and the sRGB
format codes of the containers."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import mip_filter_ref as ref
from convectionkernels_amd import api, container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_tables_are_the_restatements():
    t, u = api.srgb_tables()
    assert t.dtype == np.uint16 and u.dtype == np.uint32 and t.shape == (256,) and u.shape == (255,)
    assert (t == ref.T).all() and (u == ref.U).all()
    lib = api.load_library()
    assert lib.cvttmi_srgb_tables(None, u.ctypes.data) == -1 and lib.cvttmi_srgb_tables(t.ctypes.data, None) == -1
    assert {"cvttmi_srgb_tables", "cvttmi_build_mips_filtered_device"} <= set(api.exported_symbols())


def test_generator_renders_the_committed_header():
    spec = importlib.util.spec_from_file_location("gen_srgb", os.path.join(ROOT, "tools", "gen_srgb_tables.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    for target, text in m.render().items():
        assert open(os.path.join(ROOT, target)).read() == text, target
    t, u, c = m.build()
    assert (np.array(t) == ref.T).all() and (np.array(u) == ref.U).all()
    # the derived table of the kernels: encode at the start of every bucket of 64, and at most one threshold per bucket
    assert (np.array(c) == ref.encode(64 * np.arange(4096))).all() and np.diff(ref.U.astype(np.int64)).min() > 64


def test_tables_increase_and_equal_texels_reproduce_themselves():
    t, u = ref.T.astype(np.int64), ref.U.astype(np.int64)
    assert (np.diff(t) > 0).all() and np.diff(t).min() == 19 and t[0] == 0 and t[255] == 65535
    assert (np.diff(u) > 0).all() and u[0] > 0 and u[-1] <= 4 * 65535
    assert (ref.encode(4 * t) == np.arange(256)).all()
    # ... with room: 4 T[v] is at least 37 from the thresholds on either side
    assert (4 * t[1:] - u).min() >= 37 and (u - 4 * t[:-1]).min() >= 37


def test_encode_is_monotone_over_every_sum():
    e = ref.encode(np.arange(4 * 65535 + 1))
    assert e[0] == 0 and e[-1] == 255 and (np.diff(e) >= 0).all() and np.diff(e).max() == 1


@functools.lru_cache(maxsize=None)
def _random_quads():
    rng = np.random.default_rng(20261019)
    q = rng.integers(0, 256, (4, 2_000_000, 4), dtype=np.uint8)
    q[:, :1000, 3] = 0     # all-transparent quads
    q[:, 1000:2000, 3] = 255
    q[1:, 2000:3000, 3] = 0  # one texel carries all the weight
    return tuple(q)


def _as_level(a, b, c, d):
    """N quads -> a (2, 2N, 4) image whose level 1 is the N outputs"""
    img = np.empty((2, 2 * len(a), 4), a.dtype)
    img[0, 0::2], img[0, 1::2], img[1, 0::2], img[1, 1::2] = a, b, c, d
    return img


def _compare(got, want, where=None, what=""):
    diff = np.abs(got.astype(np.int64) - want)
    if where is not None:
        diff = diff[where]
    share = float((diff != 0).mean())
    print("%s: max difference %d, differing %.4f %%" % (what, diff.max(), 100 * share))
    assert diff.max() <= 1 and share <= 0.01, what


def test_restatement_against_float64_on_random_quads():
    a, b, c, d = _random_quads()
    img = _as_level(a, b, c, d)
    _compare(ref.downsample(img, "srgb")[0, :, :3], ref.float64_srgb(a, b, c, d), what="srgb")
    _compare(ref.downsample(img, "srgb+alpha")[0, :, :3], ref.float64_srgb(a, b, c, d, weighted=True), what="srgb+alpha")
    _compare(ref.downsample(img, "box+alpha")[0, :, :3], ref.float64_box_weighted(a, b, c, d), what="box+alpha")
    want, defined = ref.float64_normal(a, b, c, d)
    _compare(ref.downsample(img, "normal")[0, :, :3], want, where=defined, what="normal")


def test_restatement_against_float64_on_every_pair():
    x, y = (v.reshape(-1).astype(np.uint8) for v in np.meshgrid(np.arange(256), np.arange(256)))
    a = np.stack([x, x, x, np.full_like(x, 255)], -1)
    c = np.stack([y, y, y, np.full_like(y, 255)], -1)
    _compare(ref.downsample(_as_level(a, a, c, c), "srgb")[0, :, :3], ref.float64_srgb(a, a, c, c), what="srgb (a, a, b, b)")
    rng = np.random.default_rng(7)
    a[:, 3], c[:, 3] = rng.integers(0, 256, len(a)), rng.integers(0, 256, len(a))
    a2, c2 = a.copy(), c.copy()
    a2[:, 3], c2[:, 3] = rng.integers(0, 256, len(a)), rng.integers(0, 256, len(a))
    _compare(ref.downsample(_as_level(a, a2, c, c2), "srgb+alpha")[0, :, :3], ref.float64_srgb(a, a2, c, c2, weighted=True),
             what="srgb+alpha (a, a, b, b)")
    want, defined = ref.float64_normal(a, a, c, c)
    _compare(ref.downsample(_as_level(a, a, c, c), "normal")[0, :, :3], want, where=defined, what="normal (a, a, b, b)")


def _quad(a, b, c, d, dtype=np.uint8):
    return np.array([[a, b], [c, d]], dtype)


def test_checkerboard():
    img = _quad((0,) * 4, (255,) * 4, (255,) * 4, (0,) * 4)
    assert ref.downsample(img, "srgb")[0, 0].tolist() == [188, 188, 188, 128]
    assert ref.downsample(img, "box")[0, 0].tolist() == [128, 128, 128, 128]


@pytest.mark.parametrize("filt", ["box+alpha", "srgb+alpha"])
def test_transparent_texels_carry_no_colour(filt):
    img = _quad((255, 0, 0, 0), (255, 0, 0, 0), (0, 255, 0, 255), (255, 0, 0, 0))
    assert ref.downsample(img, filt)[0, 0].tolist() == [0, 255, 0, 64]
    # nothing to weight by: the unweighted filter's result
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (6, 10, 4), dtype=np.uint8)
    img[..., 3] = 0
    assert (ref.downsample(img, filt) == ref.downsample(img, filt.split("+")[0])).all()


def test_normal_map_rules_by_hand():
    # the unit axes come back as themselves, shortened sums are stretched to unit length
    z = (128, 128, 255, 7)
    assert ref.downsample(_quad(z, z, z, z), "normal")[0, 0].tolist() == [128, 128, 255, 7]
    tilt = _quad((255, 128, 128, 0), (128, 128, 255, 0), (255, 128, 128, 0), (128, 128, 255, 0))
    assert ref.downsample(tilt, "normal")[0, 0].tolist() == [218, 128, 218, 0]  # floor(127.5 / sqrt(2) + 128) = 218; box gives 192
    # opposite vectors cancel: Q == 0, the box rule
    flat = _quad((0, 0, 0, 9), (255, 255, 255, 9), (255, 255, 255, 9), (0, 0, 0, 9))
    assert ref.downsample(flat, "normal")[0, 0].tolist() == [128, 128, 128, 9]
    s = _quad((0, 0, 127, 5), (0, 0, 127, 5), (0, 0, -128, 5), (0, 0, 127, 5), np.int8)
    assert ref.downsample(s, "normal")[0, 0].tolist() == [0, 0, 127, 5]  # -128 counts as -127
    assert ref.downsample(np.zeros((2, 2, 4), np.int8), "normal")[0, 0].tolist() == [0, 0, 0, 0]


# ---- containers ----

SRGB_CODES = {"etc2": (0x9275, None), "etc2punchthrough": (0x9277, None), "etc2rgba": (0x9279, None), "bc1": (0x8C4D, 72),
              "bc2": (0x8C4E, 75), "bc3": (0x8C4F, 78), "bc7": (0x8E8D, 99)}


def _levels(fmt, w, h, count):
    rng = np.random.default_rng(len(fmt))
    per = container.FORMATS[fmt][0]
    return [rng.integers(0, 256, (((lw + 3) // 4) * ((lh + 3) // 4), per), dtype=np.uint8) for lw, lh in container.mip_sizes(w, h, count)]


@pytest.mark.parametrize("fmt", sorted(SRGB_CODES))
def test_srgb_mark_round_trips(fmt, tmp_path):
    import struct
    w, h = 37, 10
    levels = _levels(fmt, w, h, 6)
    gl, dxgi = SRGB_CODES[fmt]
    kinds = [(container.ktx_bytes, container.ktx_mips_bytes, container.read_ktx, container.read_ktx_mips, container.write_ktx,
              container.write_ktx_mips, 28, gl)]
    if dxgi is not None:
        kinds.append((container.dds_bytes, container.dds_mips_bytes, container.read_dds, container.read_dds_mips, container.write_dds,
                      container.write_dds_mips, 128, dxgi))
    for one_bytes, mips_bytes, read_one, read_mips, write_one, write_mips, code_at, code in kinds:
        for to_bytes, write, payload, read in ((one_bytes, write_one, levels[0], read_one), (mips_bytes, write_mips, levels, read_mips)):
            plain, marked = to_bytes(fmt, w, h, payload), to_bytes(fmt, w, h, payload, srgb=True)
            assert to_bytes(fmt, w, h, payload, srgb=False) == plain and to_bytes(fmt, w, h, payload, False) == plain
            assert struct.unpack_from("<I", marked, code_at)[0] == code
            # the mark is the only difference
            assert len(marked) == len(plain) and marked[:code_at] == plain[:code_at] and marked[code_at + 4:] == plain[code_at + 4:]
            assert container.colour_space(marked) == "srgb" and container.colour_space(plain) == "linear"
            got, want = read(marked), read(plain)
            assert got[:3] == want[:3] == (fmt, w, h)
            for x, y in zip(got[3] if isinstance(got[3], list) else [got[3]], want[3] if isinstance(want[3], list) else [want[3]]):
                assert (x == y).all()
            path = str(tmp_path / "t.bin")
            write(path, fmt, w, h, payload, srgb=True)
            assert open(path, "rb").read() == marked and container.colour_space(path) == "srgb"
            write(path, fmt, w, h, payload)
            assert open(path, "rb").read() == plain and container.colour_space(path) == "linear"
        # level 0 of a marked chain through the single-level reader
        assert (read_one(mips_bytes(fmt, w, h, levels, srgb=True))[3] == levels[0]).all()


@pytest.mark.parametrize("fmt", ["etc1", "bc4u", "bc4s", "bc5u", "bc5s", "bc6hu", "bc6hs", "r11u", "r11s"])
def test_formats_without_an_srgb_code_refuse_the_mark(fmt):
    levels = _levels(fmt, 8, 8, 2)
    writers = [(container.ktx_bytes, levels[0]), (container.ktx_mips_bytes, levels)]
    if container.FORMATS[fmt][3] is not None:
        writers += [(container.dds_bytes, levels[0]), (container.dds_mips_bytes, levels)]
    for to_bytes, payload in writers:
        with pytest.raises(ValueError):
            to_bytes(fmt, 8, 8, payload, srgb=True)
        assert container.colour_space(to_bytes(fmt, 8, 8, payload)) == "linear"
    with pytest.raises(ValueError):
        container.colour_space(b"not a texture file at all")


def test_filter_names_and_packer_arguments(tmp_path, capsys):
    from convectionkernels_amd import packer
    assert api.MIP_FILTERS == ref.FILTERS
    assert [api.mip_filter_value(n) for n in ("box", "srgb", "normal", "box+alpha", "srgb+alpha")] == [0, 1, 2, 0x100, 0x101]
    assert api.mip_filter_value(api.MIP_FILTER_SRGB | api.MIP_FILTER_ALPHA_WEIGHTED) == 0x101
    for bad in ("linear", None, -1, 1.0, True):
        with pytest.raises(api.CvttError):
            api.mip_filter_value(bad)
    # refused on the command line, before any device work
    src = str(tmp_path / "src.npy")
    np.save(src, np.zeros((4, 4, 4), np.uint8))
    out = str(tmp_path / "out.ktx")
    assert packer.main(["-format", "bc7", "-mipfilter", "cubic", src, out]) == 2
    assert packer.main(["-format", "bc7", "-mipfilter", "normal", "-alphaweight", src, out]) == 1
    assert packer.main(["-format", "bc5s", "-mipfilter", "srgb", src, out]) == 1
    assert packer.main(["-format", "bc5u", "-srgb", src, out]) == 1
    assert not os.path.exists(out)
    capsys.readouterr()
