"""Decoding into images, the parts that need no GPU: the two entry points are exported and bound, the unpacker's exit codes,
and the numpy untiling helper the GPU tests build their expected images with."""
import numpy as np
import pytest

import texture_decode_ref as R
from untile_ref import untile


def test_library_exports_the_image_decoders():
    from convectionkernels_amd import api
    lib = api.load_library()
    for name in ("cvttmi_decode_image_device", "cvttmi_decode_mips_device"):
        assert hasattr(lib, name), name
        assert name in api.exported_symbols(), name
    assert len(lib.cvttmi_decode_image_device.argtypes) == 9
    assert len(lib.cvttmi_decode_mips_device.argtypes) == 12
    # no context: CVTTMI_E_INVALID, nothing else is looked at
    assert lib.cvttmi_decode_image_device(None, 1, None, 0, 0, None, 0, 0, None) == -1
    assert lib.cvttmi_decode_mips_device(None, 1, None, 0, None, 0, 0, None, 0, 0, 0, None) == -1


@pytest.fixture
def no_device(monkeypatch):
    """any attempt to create a context fails the test"""
    from convectionkernels_amd import api

    def boom(*a, **k):
        raise AssertionError("the unpacker touched the device")
    monkeypatch.setattr(api, "default_context", boom)
    monkeypatch.setattr(api.Context, "__init__", boom)


def test_unpacker_exit_codes(tmp_path, capsys, no_device):
    from convectionkernels_amd import container, unpacker
    out = str(tmp_path / "out.npy")
    for argv in ([], ["only-one"], ["a", "b", "c"], ["-bogus", "a", out], ["-level", "a", out], ["-level", "x", "a", out],
                 ["-mips", "-level", "1", "a", out]):
        assert unpacker.main(argv) == 2, argv
        assert capsys.readouterr().err.strip() == unpacker.USAGE.strip()
    assert unpacker.USAGE.strip().startswith("python -m convectionkernels_amd.unpacker")
    # a missing file, a file that is no container, a container cut short
    assert unpacker.main([str(tmp_path / "missing.ktx"), out]) == 1
    (tmp_path / "junk.dds").write_bytes(b"not a texture at all")
    assert unpacker.main([str(tmp_path / "junk.dds"), out]) == 1
    rng = np.random.Generator(np.random.PCG64(3))
    bc1 = container.ktx_bytes("bc1", 8, 8, rng.integers(0, 256, (4, 8), dtype=np.uint8))
    (tmp_path / "short.ktx").write_bytes(bc1[:70])
    assert unpacker.main([str(tmp_path / "short.ktx"), out]) == 1
    # R11 has no image form: refused before any device work
    for fmt in ("r11u", "r11s"):
        path = tmp_path / (fmt + ".ktx")
        path.write_bytes(container.ktx_bytes(fmt, 8, 8, rng.integers(0, 256, (4, 8), dtype=np.uint8)))
        capsys.readouterr()
        assert unpacker.main([str(path), out]) == 1
        assert "no image form" in capsys.readouterr().err
        assert unpacker.main(["-mips", str(path), out]) == 1
    # a level the file does not have; a signed / half-float format into an image file
    (tmp_path / "one.ktx").write_bytes(bc1)
    assert unpacker.main(["-level", "1", str(tmp_path / "one.ktx"), out]) == 1
    (tmp_path / "s.ktx").write_bytes(container.ktx_bytes("bc4s", 8, 8, rng.integers(0, 256, (4, 8), dtype=np.uint8)))
    assert unpacker.main([str(tmp_path / "s.ktx"), str(tmp_path / "out.png")]) == 1
    assert not (tmp_path / "out.npy").exists() and not (tmp_path / "out.png").exists()


@pytest.mark.parametrize("size", [(1, 1), (5, 3), (37, 23)])
def test_untile_inverts_image_to_blocks(size):
    w, h = size
    rng = np.random.Generator(np.random.PCG64(w * 100 + h))
    for dtype, channels in ((np.uint8, 4), (np.int16, 4), (np.int8, 4)):
        info = np.iinfo(dtype)
        image = rng.integers(info.min, info.max + 1, (h, w, channels), dtype=dtype)
        blocks, valid = R.image_to_blocks(image, "bc1")
        assert blocks.shape == (((w + 3) // 4) * ((h + 3) // 4), 16, channels)
        back = untile(blocks, w, h)
        assert back.dtype == image.dtype and back.shape == image.shape and (back == image).all()
        # ... and whatever the texels outside the image hold does not matter
        noisy = blocks.copy()
        noisy[~valid] = rng.integers(info.min, info.max + 1, noisy[~valid].shape, dtype=dtype)
        assert (untile(noisy, w, h) == image).all()
        assert int(valid.sum()) == w * h
