"""Python host-side mirror of the reference's public interface for the hot path
(reference ConvectionKernels.h:73-103 ``Options``, 142-199 ``BC7EncodingPlan``, 236-277
``cvtt::Kernels``), on top of the C ABI in ``include/cvtt_mi355x.h``.

PyTorch is plumbing only (device memory / streams); numpy arrays go through the library's
own pinned staging.  There is no CPU fallback: if the HIP library cannot be loaded or no
gfx950 device is present every encode raises ``CvttError``.
"""
import ctypes
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "lib", "libcvtt_mi355x.so")

NumParallelBlocks = 8  # reference ConvectionKernels.h:71


class Flags:
    """cvtt::Flags, reference ConvectionKernels.h:33-69."""
    BC7_FastIndexing = 0x008
    BC7_TrySingleColor = 0x010
    BC7_RespectPunchThrough = 0x020
    BC6H_FastIndexing = 0x040
    S3TC_Exhaustive = 0x080
    S3TC_Paranoid = 0x100
    Uniform = 0x200
    ETC_UseFakeBT709 = 0x400
    ETC_FakeBT709Accurate = 0x800
    Fastest = BC6H_FastIndexing | BC7_FastIndexing | S3TC_Paranoid
    Faster = Fastest
    Fast = BC7_FastIndexing | S3TC_Paranoid
    Default = BC7_FastIndexing | S3TC_Paranoid
    Better = S3TC_Paranoid | S3TC_Exhaustive
    Ultra = BC7_TrySingleColor | S3TC_Paranoid | S3TC_Exhaustive | ETC_FakeBT709Accurate


class Options(ctypes.Structure):
    """cvtt::Options (44 bytes)."""
    _fields_ = [
        ("flags", ctypes.c_uint32),
        ("threshold", ctypes.c_float),
        ("redWeight", ctypes.c_float),
        ("greenWeight", ctypes.c_float),
        ("blueWeight", ctypes.c_float),
        ("alphaWeight", ctypes.c_float),
        ("refineRoundsBC7", ctypes.c_int32),
        ("refineRoundsBC6H", ctypes.c_int32),
        ("refineRoundsIIC", ctypes.c_int32),
        ("refineRoundsS3TC", ctypes.c_int32),
        ("seedPoints", ctypes.c_int32),
    ]

    def __init__(self, **kw):
        super().__init__()
        f32 = np.float32
        self.flags = Flags.Default
        self.threshold = 0.5
        self.redWeight = float(f32(0.2125) / f32(0.7154))
        self.greenWeight = 1.0
        self.blueWeight = float(f32(0.0721) / f32(0.7154))
        self.alphaWeight = 1.0
        self.refineRoundsBC7 = 2
        self.refineRoundsBC6H = 3
        self.refineRoundsIIC = 8
        self.refineRoundsS3TC = 2
        self.seedPoints = 4
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)

    def tobytes(self):
        return bytes(self)

    @classmethod
    def frombytes(cls, b):
        o = cls()
        ctypes.memmove(ctypes.addressof(o), bytes(b), ctypes.sizeof(cls))
        return o


class BC7EncodingPlan(ctypes.Structure):
    """cvtt::BC7EncodingPlan (808 bytes); default = every shape and partition, 4 seed points."""
    kNumRGBAShapes = 129
    kNumRGBShapes = 243
    _fields_ = [
        ("mode1PartitionEnabled", ctypes.c_uint64),
        ("mode2PartitionEnabled", ctypes.c_uint64),
        ("mode3PartitionEnabled", ctypes.c_uint64),
        ("mode0PartitionEnabled", ctypes.c_uint16),
        ("mode7RGBAPartitionEnabled", ctypes.c_uint64),
        ("mode7RGBPartitionEnabled", ctypes.c_uint64),
        ("mode4SP", (ctypes.c_uint8 * 2) * 4),
        ("mode5SP", ctypes.c_uint8 * 4),
        ("mode6Enabled", ctypes.c_uint8),
        ("seedPointsForShapeRGB", ctypes.c_uint8 * 243),
        ("seedPointsForShapeRGBA", ctypes.c_uint8 * 129),
        ("rgbaShapeList", ctypes.c_uint8 * 129),
        ("rgbaNumShapesToEvaluate", ctypes.c_uint8),
        ("rgbShapeList", ctypes.c_uint8 * 243),
        ("rgbNumShapesToEvaluate", ctypes.c_uint8),
    ]

    def __init__(self):
        super().__init__()
        full = 0xFFFFFFFFFFFFFFFF
        self.mode0PartitionEnabled = 0xFFFF
        self.mode1PartitionEnabled = full
        self.mode2PartitionEnabled = full
        self.mode3PartitionEnabled = full
        self.mode7RGBAPartitionEnabled = full
        self.mode7RGBPartitionEnabled = full
        self.mode6Enabled = 1
        for i in range(4):
            self.mode4SP[i][0] = 4
            self.mode4SP[i][1] = 4
            self.mode5SP[i] = 4
        for i in range(243):
            self.rgbShapeList[i] = i
            self.seedPointsForShapeRGB[i] = 4
        for i in range(129):
            self.rgbaShapeList[i] = i
            self.seedPointsForShapeRGBA[i] = 4
        self.rgbNumShapesToEvaluate = 243
        self.rgbaNumShapesToEvaluate = 129

    def tobytes(self):
        return bytes(self)

    @classmethod
    def frombytes(cls, b):
        o = cls()
        ctypes.memmove(ctypes.addressof(o), bytes(b), ctypes.sizeof(cls))
        return o


class BC7FineTuningParams(ctypes.Structure):
    """cvtt::BC7FineTuningParams (285 bytes): seed points (0 = off) per mode and partition / rotation / index selector;
    default = 4 everywhere."""
    _fields_ = [
        ("mode0SP", ctypes.c_uint8 * 16),
        ("mode1SP", ctypes.c_uint8 * 64),
        ("mode2SP", ctypes.c_uint8 * 64),
        ("mode3SP", ctypes.c_uint8 * 64),
        ("mode4SP", (ctypes.c_uint8 * 2) * 4),
        ("mode5SP", ctypes.c_uint8 * 4),
        ("mode6SP", ctypes.c_uint8),
        ("mode7SP", ctypes.c_uint8 * 64),
    ]

    def __init__(self):
        super().__init__()
        ctypes.memset(ctypes.addressof(self), 4, ctypes.sizeof(self))

    def tobytes(self):
        return bytes(self)

    @classmethod
    def frombytes(cls, b):
        o = cls()
        ctypes.memmove(ctypes.addressof(o), bytes(b), ctypes.sizeof(cls))
        return o


assert ctypes.sizeof(Options) == 44
assert ctypes.sizeof(BC7EncodingPlan) == 808
assert ctypes.sizeof(BC7FineTuningParams) == 285


class CvttError(RuntimeError):
    pass


_EXPORTS = (
    "cvttmi_source_sha256", "cvttmi_default_options", "cvttmi_default_bc7_plan", "cvttmi_create", "cvttmi_destroy",
    "cvttmi_last_error", "cvttmi_set_rcp_table", "cvttmi_get_rcp_table",
    "cvttmi_encode_bc7_device", "cvttmi_encode_bc7", "cvttmi_timing_enable", "cvttmi_timing_read",
    "cvttmi_set_exhaustive", "cvttmi_encode_bc1_device", "cvttmi_encode_bc1",
    "cvttmi_encode_bc6h_device", "cvttmi_encode_bc6h",
    "cvttmi_encode_etc2_device", "cvttmi_encode_etc2_rgba_device", "cvttmi_encode_etc2_alpha_device",
    "cvttmi_encode_etc2", "cvttmi_encode_etc2_rgba", "cvttmi_encode_etc2_alpha",
    "cvttmi_tiled_block_count", "cvttmi_tile_image_device", "cvttmi_compact_rows_device",
    "cvttmi_selftest_arith",
    "cvttmi_encode_etc2_alpha11_device", "cvttmi_encode_etc2_alpha11",
    "cvttmi_encode_bc2_device", "cvttmi_encode_bc3_device", "cvttmi_encode_bc4_device", "cvttmi_encode_bc5_device",
    "cvttmi_encode_bc2", "cvttmi_encode_bc3", "cvttmi_encode_bc4", "cvttmi_encode_bc5",
    "cvttmi_decode_bc7_device", "cvttmi_decode_bc7", "cvttmi_decode_bc6h_device", "cvttmi_decode_bc6h",
    "cvttmi_encode_etc1_device", "cvttmi_encode_etc1",
    "cvttmi_encode_etc2_punchthrough_alpha_device", "cvttmi_encode_etc2_punchthrough_alpha",
    "cvttmi_encode_etc2_with_data_device", "cvttmi_encode_etc2_with_data",
    "cvttmi_default_bc7_fine_tuning", "cvttmi_bc7_plan_from_quality", "cvttmi_bc7_plan_from_fine_tuning",
    "cvttmi_host_alloc", "cvttmi_host_free", "cvttmi_host_register", "cvttmi_host_unregister",
    "cvttmi_shard_block_rows", "cvttmi_multi_create", "cvttmi_multi_destroy", "cvttmi_multi_last_error", "cvttmi_multi_num_devices",
    "cvttmi_multi_context", "cvttmi_multi_last_shard", "cvttmi_multi_set_rcp_table", "cvttmi_multi_set_exhaustive", "cvttmi_multi_encode", "cvttmi_multi_encode_device",
    "cvttmi_encode_bc7_multi", "cvttmi_encode_bc1_multi", "cvttmi_encode_bc6h_multi", "cvttmi_encode_etc2_rgba_multi",
    "cvttmi_dropin_set_devices",
    "cvttmi_format_info", "cvttmi_encode_device", "cvttmi_encode",
    "cvttmi_mip_level_count", "cvttmi_mip_layout", "cvttmi_build_mips_device",
    "cvttmi_decode_image_device", "cvttmi_decode_mips_device",
    "cvttmi_build_mips_filtered_device", "cvttmi_srgb_tables", "cvttmi_mip_kernel_taps",
    "cvttmi_texture_layout", "cvttmi_texture_subresource", "cvttmi_build_mips_array_device", "cvttmi_encode_texture_device",
    "cvttmi_resize_taps", "cvttmi_resize_work_bytes", "cvttmi_resize_launches", "cvttmi_resize_image_device",
)

_lib = None


def _preload_hip_runtime():
    want = os.environ.get("CVTTMI_PRELOAD_HIP", "")
    if want == "0" or "torch" in sys.modules:
        return None
    cand = None
    if want:
        cand = want
    else:
        import importlib.util
        try:
            spec = importlib.util.find_spec("torch")  # locates the package without importing it
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.submodule_search_locations:
            for d in spec.submodule_search_locations:
                c = os.path.join(d, "lib", "libamdhip64.so")
                if os.path.exists(c):
                    cand = c
                    break
    if not cand:
        return None
    try:
        return ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
    except OSError:
        return None


def load_library():
    """dlopen the HIP library (loudly fails when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("CVTTMI_LIB", _LIB_PATH)  # override: A/B builds of the same library
    if not os.path.exists(path):
        raise CvttError("%s is missing: build it with `make -C convectionkernels_amd/csrc` "
                        "(or __graft_entry__.build())" % path)
    # One HIP runtime per process.  The library links against libamdhip64 by soname; PyTorch-ROCm ships a libamdhip64 of its own.
    # Loaded in the order library -> torch, the process ends up with two runtimes and the library's finds no device any more
    # (cvttmi_create = CVTTMI_E_NO_DEVICE; observed on the MI355X box, round 5).  The dynamic loader binds a soname once per
    # process, so it is enough that torch's runtime is mapped (RTLD_GLOBAL) BEFORE this library: then both use that one.
    #   * torch already imported: its runtime is there, nothing to do;
    #   * torch installed but not imported (numpy-only callers): preload just its libamdhip64.so -- no `import torch`, no
    #     multi-second start-up, no GPU initialisation -- so that a later `import torch` meets the runtime it expects;
    #   * no torch: the system runtime, as for any C / C++ caller (INTEGRATION.md "One HIP runtime per process").
    # CVTTMI_PRELOAD_HIP=<path> names the runtime to preload explicitly; CVTTMI_PRELOAD_HIP=0 turns the preload off.
    _preload_hip_runtime()
    lib = ctypes.CDLL(path)
    variant = "CVTTMI_LIB" in os.environ  # a developer's A/B library (tools/ab_*.sh) may predate the newest entry points
    for name in _EXPORTS:
        if not hasattr(lib, name) and not (variant and name == "cvttmi_source_sha256"):
            raise CvttError("symbol %s missing from %s" % (name, path))
    if hasattr(lib, "cvttmi_source_sha256"):
        lib.cvttmi_source_sha256.restype = ctypes.c_char_p
        lib.cvttmi_source_sha256.argtypes = []
    lib.cvttmi_last_error.restype = ctypes.c_char_p
    lib.cvttmi_last_error.argtypes = [ctypes.c_void_p]
    lib.cvttmi_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
    lib.cvttmi_destroy.argtypes = [ctypes.c_void_p]
    lib.cvttmi_set_rcp_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.cvttmi_get_rcp_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    P, N, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    # the encoders: the generic entry, and the named ones by signature family -- (ctx, out, blocks, numBlocks, options, extra...),
    # the _device forms with a stream behind
    lib.cvttmi_format_info.argtypes = [I, ctypes.POINTER(N), ctypes.POINTER(N), ctypes.POINTER(ctypes.c_uint32)]
    lib.cvttmi_encode.argtypes = [P, I, P, P, N, P, P, P]
    lib.cvttmi_encode_device.argtypes = [P, I, P, P, N, P, P, P, P]
    for names, extra in ((("bc1", "bc2", "bc3", "etc1", "etc2", "etc2_rgba", "etc2_alpha", "etc2_punchthrough_alpha"), []),
                         (("bc7",), [P]), (("bc4", "bc5", "bc6h"), [I]), (("etc2_with_data",), [P, I])):
        for n in names:
            getattr(lib, "cvttmi_encode_" + n).argtypes = [P, P, P, N, P] + extra
            getattr(lib, "cvttmi_encode_" + n + "_device").argtypes = [P, P, P, N, P] + extra + [P]
    lib.cvttmi_encode_etc2_alpha11.argtypes = [P, P, P, N, I, P]
    lib.cvttmi_encode_etc2_alpha11_device.argtypes = [P, P, P, N, I, P, P]
    lib.cvttmi_tiled_block_count.restype = ctypes.c_size_t
    lib.cvttmi_tiled_block_count.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.cvttmi_tile_image_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                             ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lib.cvttmi_compact_rows_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_void_p]
    lib.cvttmi_mip_level_count.restype = ctypes.c_uint32
    lib.cvttmi_mip_level_count.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.cvttmi_mip_layout.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.cvttmi_build_mips_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32,
                                             ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p]
    lib.cvttmi_build_mips_filtered_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32,
                                                      ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                                      ctypes.c_void_p]
    lib.cvttmi_srgb_tables.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.cvttmi_mip_kernel_taps.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32)]
    U = ctypes.c_uint32
    lib.cvttmi_texture_layout.argtypes = [U, U, I, U, U, U, I, P]
    lib.cvttmi_texture_subresource.argtypes = [U, U, I, U, U, U, I, U, U, ctypes.POINTER(N), ctypes.POINTER(N)]
    lib.cvttmi_build_mips_array_device.argtypes = [P, P, N, P, U, U, N, N, I, U, U, U, P]
    lib.cvttmi_encode_texture_device.argtypes = [P, I, P, N, P, U, U, N, N, U, U, U, I, P, P, P, P, N, P]
    lib.cvttmi_resize_taps.argtypes = [U, U, U, P, P, ctypes.POINTER(U)]
    lib.cvttmi_resize_work_bytes.argtypes = [U, U, U, U, I, U, U, ctypes.POINTER(N)]
    lib.cvttmi_resize_launches.argtypes = [U, U, U, U, I, U, ctypes.POINTER(U)]
    lib.cvttmi_resize_image_device.argtypes = [P, P, U, U, N, N, P, U, U, N, N, I, U, U, P, N, P]
    lib.cvttmi_decode_bc7_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.cvttmi_decode_bc7.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.cvttmi_decode_bc6h_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    lib.cvttmi_decode_bc6h.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    lib.cvttmi_decode_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.cvttmi_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.cvttmi_measure_error_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.cvttmi_measure_error.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                         ctypes.c_void_p, ctypes.c_void_p]
    lib.cvttmi_measure_image_error_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32,
                                                      ctypes.c_uint32, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_void_p]
    lib.cvttmi_decode_image_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p,
                                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.cvttmi_decode_mips_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                                              ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.cvttmi_psnr.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    lib.cvttmi_psnr.restype = ctypes.c_double
    lib.cvttmi_selftest_arith.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.POINTER(ctypes.c_uint64)]
    lib.cvttmi_bc7_plan_from_quality.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.cvttmi_bc7_plan_from_fine_tuning.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.cvttmi_default_bc7_fine_tuning.argtypes = [ctypes.c_void_p]
    lib.cvttmi_host_alloc.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    lib.cvttmi_host_free.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.cvttmi_host_register.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    lib.cvttmi_host_unregister.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.cvttmi_timing_enable.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.cvttmi_set_exhaustive.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.cvttmi_timing_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(lib, "cvttmi_multi_create"):
        lib.cvttmi_shard_block_rows.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
        lib.cvttmi_multi_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_int]
        lib.cvttmi_multi_destroy.argtypes = [ctypes.c_void_p]
        lib.cvttmi_multi_last_error.restype = ctypes.c_char_p
        lib.cvttmi_multi_last_error.argtypes = [ctypes.c_void_p]
        lib.cvttmi_multi_num_devices.argtypes = [ctypes.c_void_p]
        lib.cvttmi_multi_last_shard.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
        lib.cvttmi_multi_set_rcp_table.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        lib.cvttmi_multi_set_exhaustive.argtypes = [ctypes.c_void_p, ctypes.c_int]
        lib.cvttmi_multi_encode_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                   ctypes.c_void_p, ctypes.c_void_p]
        lib.cvttmi_multi_encode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                            ctypes.c_void_p, ctypes.c_void_p]
        lib.cvttmi_encode_bc7_multi.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                ctypes.c_void_p, ctypes.c_void_p]
        for n in ("cvttmi_encode_bc1_multi", "cvttmi_encode_etc2_rgba_multi"):
            getattr(lib, n).argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
        lib.cvttmi_encode_bc6h_multi.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t,
                                                 ctypes.c_void_p, ctypes.c_int]
        lib.cvttmi_dropin_set_devices.argtypes = [ctypes.c_void_p, ctypes.c_int]
    _lib = lib
    return lib


# Decode / measure formats (include/cvtt_mi355x.h CVTTMI_FMT_*): name -> (id, packed bytes, decoded bytes, channel mask).
# Names as encode_image and container.FORMATS use them, plus "r11u" / "r11s" (EAC R11 from PixelBlockScalarS16).
TEXTURE_FORMATS = {
    "bc7": (0, 16, 64, 0xF), "bc1": (1, 8, 64, 0xF), "bc6hu": (2, 16, 128, 0x7), "bc6hs": (3, 16, 128, 0x7),
    "etc2": (4, 8, 64, 0x7), "etc2rgb": (4, 8, 64, 0x7), "etc2rgba": (5, 16, 64, 0xF), "bc2": (6, 16, 64, 0xF),
    "bc3": (7, 16, 64, 0xF), "bc4u": (8, 8, 64, 0x1), "bc4s": (9, 8, 64, 0x1), "bc5u": (10, 16, 64, 0x3),
    "bc5s": (11, 16, 64, 0x3), "etc1": (12, 8, 64, 0x7), "etc2punchthrough": (13, 8, 64, 0xF), "eac": (14, 8, 64, 0x8),
    "r11u": (15, 8, 32, 0x1), "r11s": (16, 8, 32, 0x1),
}
# What a texel of a format is (csrc/texture_formats.h, CvttTexelClass): "unorm8" unless named here.  "half": float16 RGB, no
# PSNR; "snorm8": int8; "r11": an int16 scalar, the one class without an image form.
_TEXEL_CLASS = {"bc6hu": "half", "bc6hs": "half", "bc4s": "snorm8", "bc5s": "snorm8", "r11u": "r11", "r11s": "r11"}


def texel_class(fmt):
    return _TEXEL_CLASS.get(fmt, "unorm8")


def has_image_form(fmt):
    return fmt in TEXTURE_FORMATS and texel_class(fmt) != "r11"


# pixel kinds (include/cvtt_mi355x.h CVTTMI_PIXELS_*); the SNORM kind exists for the mip filter alone
PIXELS_RGBA8, PIXELS_RGBA16F, PIXELS_RGBA8_SNORM = 0, 1, 2

# mip filters (include/cvtt_mi355x.h CVTTMI_MIP_FILTER_*) and the names build_mips / encode_mips take for them
MIP_FILTER_BOX, MIP_FILTER_SRGB, MIP_FILTER_NORMAL, MIP_FILTER_ALPHA_WEIGHTED = 0, 1, 2, 0x100
MIP_FILTERS = {"box": MIP_FILTER_BOX, "srgb": MIP_FILTER_SRGB, "normal": MIP_FILTER_NORMAL,
               "box+alpha": MIP_FILTER_BOX | MIP_FILTER_ALPHA_WEIGHTED, "srgb+alpha": MIP_FILTER_SRGB | MIP_FILTER_ALPHA_WEIGHTED}


def mip_filter_value(filter):
    """a filter name of MIP_FILTERS, or a MIP_FILTER_* value (flag included) -> the value the library takes"""
    if isinstance(filter, str):
        if filter not in MIP_FILTERS:
            raise CvttError("unknown mip filter %r (one of %s)" % (filter, ", ".join(MIP_FILTERS)))
        return MIP_FILTERS[filter]
    if isinstance(filter, bool) or not isinstance(filter, int) or not 0 <= filter <= 0xFFFFFFFF:
        raise CvttError("mip filter must be a name or a MIP_FILTER_* value, got %r" % (filter,))
    return filter


# mip kernels and wrap modes (include/cvtt_mi355x.h CVTTMI_MIP_KERNEL_*, CVTTMI_MIP_WRAP_*): two more fields of the filter word
MIP_KERNELS = {"triangle": 0x10, "mitchell": 0x20, "lanczos3": 0x30, "kaiser": 0x40}
MIP_WRAPS = {"clamp": 0, "repeat": 0x200, "mirror": 0x400}
# the range of an RGBA16F image under a kernel or in a resize (CVTTMI_MIP_HDR_*): what the results are clamped to
MIP_HDR = {"nonnegative": 0x1000, "signed": 0x2000}


def _hdr_value(hdr):
    if hdr is None:
        return 0
    if hdr not in MIP_HDR:
        raise CvttError("unknown hdr range %r (one of %s, or None)" % (hdr, ", ".join(MIP_HDR)))
    return MIP_HDR[hdr]


def mip_filter_word(filter, kernel=None, wrap="clamp", hdr=None):
    """the `filter` value of the C calls: mip_filter_value(filter) with the kernel (a name of MIP_KERNELS or None = the 2x2 rule),
    the wrap mode (a name of MIP_WRAPS) and the range of an RGBA16F image under a kernel (a name of MIP_HDR or None) OR-ed on"""
    if kernel is not None and kernel not in MIP_KERNELS:
        raise CvttError("unknown mip kernel %r (one of %s)" % (kernel, ", ".join(MIP_KERNELS)))
    if wrap not in MIP_WRAPS:
        raise CvttError("unknown wrap mode %r (one of %s)" % (wrap, ", ".join(MIP_WRAPS)))
    return mip_filter_value(filter) | (MIP_KERNELS[kernel] if kernel is not None else 0) | MIP_WRAPS[wrap] | _hdr_value(hdr)


def mip_kernel_taps(name):
    """cvttmi_mip_kernel_taps: the Q14 tap table of a mip kernel (a name of MIP_KERNELS), int16, 4 R entries summing to 16384"""
    import numpy as np
    if name not in MIP_KERNELS:
        raise CvttError("unknown mip kernel %r (one of %s)" % (name, ", ".join(MIP_KERNELS)))
    taps, count = np.zeros(12, np.int16), ctypes.c_uint32(0)
    rc = load_library().cvttmi_mip_kernel_taps(MIP_KERNELS[name], taps.ctypes.data, ctypes.byref(count))
    if rc != 0:
        raise CvttError("cvttmi_mip_kernel_taps failed (%d)" % rc)
    return taps[:count.value].copy()


# resizing (include/cvtt_mi355x.h, "resize"): the mip kernels, and kernel code 0 = an area-average box
RESIZE_KERNELS = dict(MIP_KERNELS, box=0)
RESIZE_RULES = {"box": MIP_FILTER_BOX, "srgb": MIP_FILTER_SRGB, "normal": MIP_FILTER_NORMAL}


def resize_filter_word(kernel="lanczos3", filter="box", wrap="clamp", hdr=None):
    """the `filter` value of the resize calls: rule (a name of RESIZE_RULES or its value) | kernel (a name of RESIZE_KERNELS) | wrap
    | the range of an RGBA16F image (a name of MIP_HDR or None)"""
    if kernel not in RESIZE_KERNELS:
        raise CvttError("unknown resize kernel %r (one of %s)" % (kernel, ", ".join(RESIZE_KERNELS)))
    if wrap not in MIP_WRAPS:
        raise CvttError("unknown wrap mode %r (one of %s)" % (wrap, ", ".join(MIP_WRAPS)))
    if isinstance(filter, str) and filter not in RESIZE_RULES:
        raise CvttError("unknown resize filter %r (one of %s)" % (filter, ", ".join(RESIZE_RULES)))
    return mip_filter_value(filter) | RESIZE_KERNELS[kernel] | MIP_WRAPS[wrap] | _hdr_value(hdr)


def resize_taps(src, dst, kernel, wrap="clamp"):
    """cvttmi_resize_taps: the tables of one axis of `src` texels resized to `dst` under a kernel (a name of RESIZE_KERNELS) ->
    (first, weights): first[x], int32, the unwrapped source coordinate of output x's tap 0; weights[x, k], int16 Q14, every row
    summing to 16384.  `wrap` does not change the table: tap k reads first[x] + k wrapped by it."""
    import numpy as np
    lib, n = load_library(), ctypes.c_uint32(0)
    word = resize_filter_word(kernel, "box", wrap)
    src, dst = _u32(src, "src"), _u32(dst, "dst")
    rc = lib.cvttmi_resize_taps(src, dst, word, None, None, ctypes.byref(n))
    if rc != 0:
        raise CvttError("cvttmi_resize_taps(%d -> %d) failed (%d): sizes are 1 .. 65535" % (src, dst, rc))
    weights, first = np.zeros((dst, n.value), np.int16), np.zeros(dst, np.int32)
    rc = lib.cvttmi_resize_taps(src, dst, word, weights.ctypes.data, first.ctypes.data, ctypes.byref(n))
    if rc != 0:
        raise CvttError("cvttmi_resize_taps(%d -> %d) failed (%d): the table does not keep the sums inside int32" % (src, dst, rc))
    return first, weights


def resize_launches(src_w, src_h, dst_w, dst_h, kernel="lanczos3", filter="box", signed=False, hdr=None):
    """cvttmi_resize_launches: 1 where Context.resize of these sizes runs as one launch through LDS, 2 where it goes through an
    intermediate in its work space.  hdr: a name of MIP_HDR = an RGBA16F image under that range"""
    n = ctypes.c_uint32(0)
    rc = load_library().cvttmi_resize_launches(_u32(src_w, "src_w"), _u32(src_h, "src_h"), _u32(dst_w, "dst_w"), _u32(dst_h, "dst_h"),
                                               PIXELS_RGBA16F if hdr is not None else PIXELS_RGBA8_SNORM if signed else PIXELS_RGBA8,
                                               resize_filter_word(kernel, filter, hdr=hdr), ctypes.byref(n))
    if rc != 0:
        raise CvttError("cvttmi_resize_launches failed (%d)" % rc)
    return n.value


def srgb_tables():
    """cvttmi_srgb_tables: (T, U) of the sRGB mip filter -- T[v], v = 0..255, uint16 linear light of a byte; U[k - 1], k = 1..255,
    uint32, the smallest sum of four T that encodes to k or more"""
    import numpy as np
    t, u = np.zeros(256, np.uint16), np.zeros(255, np.uint32)
    rc = load_library().cvttmi_srgb_tables(t.ctypes.data, u.ctypes.data)
    if rc != 0:
        raise CvttError("cvttmi_srgb_tables failed (%d)" % rc)
    return t, u


class MipLevel(ctypes.Structure):
    """byte image of cvttmi_mip_level: a level's size and its place in the pyramid, the tiled and the packed buffer"""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("byteOffset", ctypes.c_size_t),
                ("rowPitchBytes", ctypes.c_size_t), ("firstTile", ctypes.c_size_t), ("tileCount", ctypes.c_size_t),
                ("firstBlock", ctypes.c_size_t), ("blockCount", ctypes.c_size_t), ("packedByteOffset", ctypes.c_size_t)]


class MipLayout(list):
    """cvttmi_mip_layout: a list of MipLevel, one per level, with the three totals -- bytes of the pyramid (levels 1..), blocks
    of the tiled buffer, blocks of the packed output"""
    pyramid_bytes = tile_count = block_count = 0


def mip_level_count(width, height):
    """cvttmi_mip_level_count: levels of the full chain down to 1x1; 0 when a size is 0"""
    return int(load_library().cvttmi_mip_level_count(int(width), int(height)))


def mip_layout(width, height, pixel_bytes, bytes_per_block, levels=None):
    """cvttmi_mip_layout for an image of `pixel_bytes` per texel (4 = RGBA8, 8 = RGBA16F) and a format of `bytes_per_block`;
    levels: None = the full chain.  Needs no device."""
    lib = load_library()
    levels = mip_level_count(width, height) if levels is None else int(levels)
    kind = {4: PIXELS_RGBA8, 8: PIXELS_RGBA16F}.get(pixel_bytes, -1)
    table = (MipLevel * (max(levels, 0) + 1))()
    rc = lib.cvttmi_mip_layout(int(width), int(height), kind, int(bytes_per_block), max(levels, 0), table)
    if rc != 0:
        raise CvttError("cvttmi_mip_layout(%d x %d, %d bytes per texel, %d bytes per block, %d levels) failed (%d)"
                        % (width, height, pixel_bytes, bytes_per_block, levels, rc))
    out = MipLayout(table[:levels])
    end = table[levels]
    out.pyramid_bytes, out.tile_count, out.block_count = int(end.byteOffset), int(end.firstTile), int(end.firstBlock)
    return out


# texture arrays and cube maps (include/cvtt_mi355x.h CVTTMI_ORDER_*): the packed output's order and its names
ORDER_LAYER_MAJOR, ORDER_LEVEL_MAJOR = 0, 1
ORDERS = {"layer": ORDER_LAYER_MAJOR, "level": ORDER_LEVEL_MAJOR}


def order_value(order):
    """"layer" (DDS order) / "level" (KTX order), or an ORDER_* value -> the value the library takes (unknown integers are the
    library's to refuse)"""
    if isinstance(order, str):
        if order not in ORDERS:
            raise CvttError("unknown order %r (one of %s)" % (order, ", ".join(ORDERS)))
        return ORDERS[order]
    if isinstance(order, bool) or not isinstance(order, int) or not -(1 << 31) <= order < (1 << 31):
        raise CvttError("order must be a name or an ORDER_* value, got %r" % (order,))
    return order


class TextureSizes(ctypes.Structure):
    """byte image of cvttmi_texture_sizes: what cvttmi_texture_layout reports for `layers` images with `levels` levels each"""
    _fields_ = [("pyramidLayerBytes", ctypes.c_size_t), ("pyramidBytes", ctypes.c_size_t), ("tilesPerLayer", ctypes.c_size_t),
                ("tiles", ctypes.c_size_t), ("blocksPerLayer", ctypes.c_size_t), ("blocks", ctypes.c_size_t), ("workBytes", ctypes.c_size_t)]


def _pixel_kind(pixel_bytes):
    return {4: PIXELS_RGBA8, 8: PIXELS_RGBA16F}.get(pixel_bytes, -1)


def _u32(value, what):
    value = int(value)
    if not 0 <= value <= 0xFFFFFFFF:
        raise CvttError("%s = %d is no uint32" % (what, value))
    return value


def texture_layout(width, height, pixel_bytes, bytes_per_block, levels=None, layers=1, order="layer"):
    """cvttmi_texture_layout: the sizes of a texture of `layers` images of `pixel_bytes` per texel (4 = RGBA8, 8 = RGBA16F), each
    with `levels` levels (None = the full chain), for a format of `bytes_per_block` -> TextureSizes.  Needs no device."""
    levels = mip_level_count(width, height) if levels is None else levels
    out = TextureSizes()
    rc = load_library().cvttmi_texture_layout(_u32(width, "width"), _u32(height, "height"), _pixel_kind(pixel_bytes), _u32(bytes_per_block, "bytes_per_block"),
                                              _u32(levels, "levels"), _u32(layers, "layers"), order_value(order), ctypes.byref(out))
    if rc != 0:
        raise CvttError("cvttmi_texture_layout(%d x %d, %d bytes per texel, %d bytes per block, %d levels, %d layers, order %r) failed (%d)"
                        % (width, height, pixel_bytes, bytes_per_block, levels, layers, order, rc))
    return out


def texture_subresource(width, height, pixel_bytes, bytes_per_block, levels, layers, order, layer, level):
    """cvttmi_texture_subresource: (first block, block count) of (layer, level) in the packed output of a texture in `order`.
    levels: None = the full chain.  Needs no device."""
    levels = mip_level_count(width, height) if levels is None else levels
    first, count = ctypes.c_size_t(), ctypes.c_size_t()
    rc = load_library().cvttmi_texture_subresource(_u32(width, "width"), _u32(height, "height"), _pixel_kind(pixel_bytes),
                                                   _u32(bytes_per_block, "bytes_per_block"), _u32(levels, "levels"), _u32(layers, "layers"),
                                                   order_value(order), _u32(layer, "layer"), _u32(level, "level"), ctypes.byref(first), ctypes.byref(count))
    if rc != 0:
        raise CvttError("cvttmi_texture_subresource(%d x %d, %d levels, %d layers, order %r, layer %d, level %d) failed (%d)"
                        % (width, height, levels, layers, order, layer, level, rc))
    return int(first.value), int(count.value)


@functools.lru_cache(maxsize=64)
def _texture_places(width, height, pixel_bytes, bytes_per_block, levels, layers, order):
    """texture_subresource of every subresource, kept for the shapes last used, as (first block of layer 0, blocks from one layer
    to the next, block count) per level: in both orders a level's layers are evenly spaced, which is checked here, not assumed"""
    places = [[texture_subresource(width, height, pixel_bytes, bytes_per_block, levels, layers, order, layer, level)
               for level in range(levels)] for layer in range(layers)]
    out = []
    for level in range(levels):
        first, count = places[0][level]
        step = places[1][level][0] - first if layers > 1 else count
        if any(places[layer][level] != (first + layer * step, count) for layer in range(layers)) or step < count:
            raise CvttError("cvttmi_texture_subresource: the layers of level %d are not evenly spaced" % level)
        out.append((first, step, count))
    return tuple(out)


class TextureBlocks(list):
    """What Context.encode_texture returns: [layer][level] -> the (blocks, bytes per block) uint8 view of that subresource.
    base: the ONE allocation all of them are views of, (all blocks, bytes per block), in `order` -- what a container of that
    order stores behind its header."""
    base = None
    order = "layer"


class ErrorTotals(ctypes.Structure):
    """byte image of cvttmi_error_totals"""
    _fields_ = [("sse", ctypes.c_uint64 * 4), ("sseHdr", ctypes.c_double * 4), ("texels", ctypes.c_uint64),
                ("channelMask", ctypes.c_uint32), ("format", ctypes.c_int32)]


def psnr_of_totals(totals, channel_mask=0):
    """cvttmi_psnr: dB over the channels of channel_mask (0 = the format's)"""
    return float(load_library().cvttmi_psnr(ctypes.addressof(totals), int(channel_mask)))


class ErrorReport:
    """Result of Context.measure_error / measure_image: per-channel SSE and MSE (R, G, B, A; channels the format does not
    store are 0 and not in `channels`), the texels counted per channel, psnr(), and the per-block values when asked for."""
    _CH = {"r": 1, "g": 2, "b": 4, "a": 8}

    def __init__(self, fmt, totals, per_block=None):
        self.format = fmt
        self.totals = totals
        self.channel_mask = int(totals.channelMask)
        self.texels = int(totals.texels)
        hdr = texel_class(fmt) == "half"
        self.sse = [float(totals.sseHdr[c]) if hdr else int(totals.sse[c]) for c in range(4)]
        self.mse = [(s / self.texels if self.texels else float("nan")) if (self.channel_mask >> c) & 1 else 0.0
                    for c, s in enumerate(self.sse)]
        self.channels = "".join(ch for ch, bit in self._CH.items() if self.channel_mask & bit)
        self.per_block = per_block

    def psnr(self, channels=None):
        """dB over `channels` ("rgb", "a", a mask, None = every channel the format stores); NaN for BC6H"""
        mask = channels if isinstance(channels, int) else sum(self._CH[c] for c in (channels or "").lower())
        return psnr_of_totals(self.totals, mask)

    def __repr__(self):
        return "ErrorReport(%s, mse=%s, texels=%d, psnr=%.3f)" % (self.format, self.mse, self.texels, self.psnr())


def library_source_sha256():
    """Build identity compiled into the loaded library (csrc/Makefile: SHA-256 over the kernel and shim sources, the public
    headers and the compiler flags).  The same for every build of the same tree, whatever the build directory; profiles/
    summaries carry it and bench.py quotes their counters only when it matches."""
    lib = load_library()
    return lib.cvttmi_source_sha256().decode() if hasattr(lib, "cvttmi_source_sha256") else ""


def library_fatbin_sha256(path=None):
    """SHA-256 of the device code (.hip_fatbin section) of the library that load_library() uses: identifies the kernel
    objects a profile was taken with (bench.py only quotes profiles/rNN/summary.json counters when it matches)."""
    import hashlib
    import struct
    path = path or os.environ.get("CVTTMI_LIB", _LIB_PATH)
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2:
        return hashlib.sha256(data).hexdigest()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    stroff = secs[shstrndx][4]
    for name_off, _type, _flags, _addr, off, size, *_ in secs:
        end = data.index(b"\0", stroff + name_off)
        if data[stroff + name_off:end] == b".hip_fatbin":
            return hashlib.sha256(data[off:off + size]).hexdigest()
    return hashlib.sha256(data).hexdigest()


def exported_symbols():
    return _EXPORTS


class Context:
    """One encoder context on one HIP device (tables in HBM, staging and work buffers, rcp table).

    Concurrency: a context owns ONE set of device work buffers (the BC7 hand-over list and punch-through table, the host-path
    staging ring).  The calls that use them are ordered by the library itself when they arrive on
    different streams (cvtt_mi355x.h "Streams"; calls that use no shared work space are simply queued on their stream), the
    host side of every call on a context is serialised by a mutex in the library, and the host-pointer calls additionally by
    a lock here, so sharing a context between threads or streams is safe but not concurrent -- use one Context per worker
    thread (they are cheap: ~10 KB of tables + the work buffers) to overlap independent jobs."""

    def __init__(self, device=0):
        import threading
        self._host_lock = threading.Lock()
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        rc = self._lib.cvttmi_create(ctypes.byref(self._h), int(device))
        if rc != 0:
            raise CvttError("cvttmi_create(device=%d) failed with %d (no gfx950 device?)" % (device, rc))
        self.device = int(device)

    def close(self):
        if self._h:
            self._lib.cvttmi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            msg = self._lib.cvttmi_last_error(self._h)
            raise CvttError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    # -- argument checks shared by every entry point: a wrong buffer must raise here, never reach a kernel or memcpy --
    @staticmethod
    def _host_out(out, n, out_bytes, dtype=np.uint8, shape=None):
        """the caller's numpy result buffer, or a fresh one"""
        if out is None:
            return np.empty(shape if shape is not None else (n, out_bytes), dtype)
        need = n * out_bytes
        if not (isinstance(out, np.ndarray) and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and out.nbytes == need
                and out.dtype.itemsize == np.dtype(dtype).itemsize):
            raise CvttError("out must be a writable C-contiguous numpy array of exactly %d bytes (%d blocks x %d), %d-byte elements"
                            % (need, n, out_bytes, np.dtype(dtype).itemsize))
        return out

    def _device_in(self, t, what="blocks"):
        import torch
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise CvttError("%s must be a numpy array or a CUDA tensor (got %s)" % (what, type(t).__name__ if not isinstance(t, torch.Tensor) else "a CPU tensor"))
        if t.device.index != self.device:
            raise CvttError("%s lives on cuda:%d but this context was created for cuda:%d" % (what, t.device.index, self.device))
        return t.contiguous()

    def _device_out(self, out, n, out_bytes, like, dtype=None, shape=None):
        """the caller's CUDA result tensor, or a fresh one on the input's device"""
        import torch
        dtype = dtype or torch.uint8
        if out is None:
            return torch.empty(shape if shape is not None else (n, out_bytes), dtype=dtype, device=like.device)
        need = n * out_bytes
        if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == like.device and out.is_contiguous()
                and out.numel() * out.element_size() == need and out.element_size() == torch.empty((), dtype=dtype).element_size()):
            raise CvttError("out must be a contiguous CUDA tensor on %s of exactly %d bytes (%d blocks x %d)" % (like.device, need, n, out_bytes))
        return out

    def _stream(self, stream, device):
        import torch
        return torch.cuda.current_stream(device).cuda_stream if stream is None else stream

    # -- reciprocal table (host RCPPS probe; see include/cvtt_mi355x.h) --
    def get_rcp_table(self):
        out = np.zeros(17, np.float32)
        self._check(self._lib.cvttmi_get_rcp_table(self._h, out.ctypes.data), "get_rcp_table")
        return out

    def set_rcp_table(self, lut):
        lut = np.ascontiguousarray(lut, np.float32)
        assert lut.size == 17
        self._check(self._lib.cvttmi_set_rcp_table(self._h, lut.ctypes.data), "set_rcp_table")

    # -- page-locked host memory for the host-pointer (numpy) entry points --
    def host_empty(self, shape, dtype=np.uint8):
        """numpy array in page-locked memory (cvttmi_host_alloc): the numpy entry points move it over PCIe in place,
        pipelined with the search, instead of staging it through a copy.  Freed when the array and its views are gone."""
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape)) * dtype.itemsize
        p = ctypes.c_void_p()
        self._check(self._lib.cvttmi_host_alloc(self._h, ctypes.byref(p), nbytes), "host_alloc")
        lib, addr = self._lib, p.value

        class _Owner:
            def __del__(self_inner):
                # without the context: the array may outlive it (cvttmi_host_free accepts NULL)
                try:
                    lib.cvttmi_host_free(None, ctypes.c_void_p(addr))
                except Exception:  # noqa
                    pass
        buf = (ctypes.c_uint8 * max(1, nbytes)).from_address(addr)
        buf._owner = _Owner()
        return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def host_register(self, array):
        """page-lock an existing C-contiguous numpy array in place (undo with host_unregister before freeing it)"""
        a = np.ascontiguousarray(array)
        if a.ctypes.data != array.ctypes.data:
            raise CvttError("array must be C-contiguous")
        self._check(self._lib.cvttmi_host_register(self._h, a.ctypes.data, a.nbytes), "host_register")

    def host_unregister(self, array):
        self._check(self._lib.cvttmi_host_unregister(self._h, array.ctypes.data), "host_unregister")

    def set_exhaustive(self, on=True):
        """search every candidate like the reference (default: exact branch-and-bound pruning)"""
        self._check(self._lib.cvttmi_set_exhaustive(self._h, 1 if on else 0), "set_exhaustive")

    # -- timing of the kernels launched by *_device calls (HIP events on the launch stream) --
    def timing_enable(self, on=True):
        self._check(self._lib.cvttmi_timing_enable(self._h, 1 if on else 0), "timing_enable")

    def timing_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_uint64()
        self._check(self._lib.cvttmi_timing_read(self._h, ctypes.byref(ms), ctypes.byref(n)), "timing_read")
        return ms.value, n.value

    # -- every encoder, by format name (cvttmi_encode / cvttmi_encode_device); the methods named after the reference's calls follow --
    def encode(self, fmt, blocks, options=None, plan=None, out=None, stream=None, compression_data=None):
        """Batched cvtt::Kernels::Encode* of format ``fmt`` (a name of TEXTURE_FORMATS).  ``blocks``: N blocks (a multiple of 8)
        in the layout the format's encoder reads -- (N,16,4) uint8 PixelBlockU8, int8 PixelBlockS8 for BC4S / BC5S, 2-byte half
        bit patterns for BC6H, (N,16) int16 PixelBlockScalarS16 for R11 -- as a numpy array (host path) or a tensor on this
        context's GPU (device path, asynchronous on ``stream`` / the current torch stream) -> (N, bytes per block) uint8.
        plan: BC7 only (None = BC7EncodingPlan()).  compression_data: ETC2 RGB / RGBA / punch-through only -- what AllocETC2Data
        returned, or the Options it was given: the chroma axes of the sector split belong to those (reference
        ConvectionKernels_ETC.cpp:3117-3145), the rest to `options`; None = allocated with `options`."""
        fid, out_bytes, in_bytes, _ = self._texture_format(fmt)
        options = options if options is not None else Options()
        if fmt == "bc7" and plan is None:
            plan = BC7EncodingPlan()
        ao = compression_data.alloc_options if isinstance(compression_data, ETC2CompressionData) else compression_data
        planp = ctypes.addressof(plan) if plan is not None else None
        aop = ctypes.addressof(ao) if ao is not None else None
        what = "encode(%s)" % fmt
        if isinstance(blocks, np.ndarray):
            # values are converted where callers hand over plain integers (BC7: uint8, R11: int16); every other array is taken
            # by its bytes (int8 for the signed formats, any 2-byte dtype for BC6H)
            b = np.ascontiguousarray(blocks, {"bc7": np.uint8, "r11u": np.int16, "r11s": np.int16}.get(fmt))
            n = b.nbytes // in_bytes
            if b.nbytes % in_bytes or n % NumParallelBlocks:
                raise CvttError("blocks must hold a multiple of 8 pixel blocks of %d bytes" % in_bytes)
            res = self._host_out(out, n, out_bytes)
            with self._host_lock:
                self._check(self._lib.cvttmi_encode(self._h, fid, res.ctypes.data, b.ctypes.data, n, ctypes.addressof(options), planp, aop), what)
            return res
        b = self._device_in(blocks)
        if fmt == "bc7" and str(b.dtype) != "torch.uint8":
            raise CvttError("blocks must be a numpy uint8 array or a CUDA uint8 tensor")
        nbytes = b.numel() * b.element_size()
        n = nbytes // in_bytes
        if nbytes % in_bytes or n % NumParallelBlocks:
            raise CvttError("blocks must hold a multiple of 8 pixel blocks of %d bytes" % in_bytes)
        res = self._device_out(out, n, out_bytes, b)
        stream = self._stream(stream, b.device)
        self._check(self._lib.cvttmi_encode_device(self._h, fid, res.data_ptr(), b.data_ptr(), n, ctypes.addressof(options), planp, aop,
                                                   ctypes.c_void_p(stream)), what)
        return res

    # -- BC7 --
    def encode_bc7(self, blocks, options=None, plan=None, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeBC7.  ``blocks``: (N,16,4) uint8 numpy array (host
        path) or a torch uint8 tensor on this context's GPU (device path, asynchronous on
        ``stream`` / the current torch stream).  N must be a multiple of 8."""
        return self.encode("bc7", blocks, options, plan, out, stream)

    # -- BC1 --
    def encode_bc1(self, blocks, options=None, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeBC1: (N,16,4) uint8 -> (N,8) uint8."""
        return self.encode("bc1", blocks, options, None, out, stream)

    # -- BC2 / BC3 / BC4 / BC5 --
    def encode_bc2(self, blocks, options=None, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeBC2: (N,16,4) uint8 -> (N,16) uint8 [explicit alpha | colour]."""
        return self.encode("bc2", blocks, options, None, out, stream)

    def encode_bc3(self, blocks, options=None, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeBC3: (N,16,4) uint8 -> (N,16) uint8 [interpolated alpha | colour]."""
        return self.encode("bc3", blocks, options, None, out, stream)

    def encode_bc4(self, blocks, options=None, signed=False, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeBC4U / EncodeBC4S (red channel; signed: int8 PixelBlockS8): -> (N,8) uint8."""
        return self.encode("bc4s" if signed else "bc4u", blocks, options, None, out, stream)

    def encode_bc5(self, blocks, options=None, signed=False, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeBC5U / EncodeBC5S (red, green): -> (N,16) uint8."""
        return self.encode("bc5s" if signed else "bc5u", blocks, options, None, out, stream)

    # -- BC6H --
    def encode_bc6h(self, blocks, options=None, signed=False, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeBC6HU / EncodeBC6HS: (N,16,4) half bit patterns (int16 /
        uint16 / float16 numpy array, or a CUDA tensor of 2-byte elements) -> (N,16) uint8."""
        return self.encode("bc6hs" if signed else "bc6hu", blocks, options, None, out, stream)

    # -- ETC1 / ETC2 --
    def encode_etc1(self, blocks, options=None, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeETC1: (N,16,4) uint8 -> (N,8) uint8."""
        return self.encode("etc1", blocks, options, None, out, stream)

    def encode_etc2(self, blocks, options=None, out=None, stream=None, compression_data=None):
        """Batched cvtt::Kernels::EncodeETC2 (RGB): (N,16,4) uint8 -> (N,8) uint8.  compression_data: what AllocETC2Data
        returned (or the Options it was given); None = allocated with `options`."""
        return self.encode("etc2", blocks, options, None, out, stream, compression_data)

    def encode_etc2_punchthrough_alpha(self, blocks, options=None, out=None, stream=None, compression_data=None):
        """Batched cvtt::Kernels::EncodeETC2PunchthroughAlpha: (N,16,4) uint8 -> (N,8) uint8 (RGB8A1 blocks; a pixel is
        transparent when its alpha is below floor(clamp(options.threshold, 0, 1) * 255 + 1))."""
        return self.encode("etc2punchthrough", blocks, options, None, out, stream, compression_data)

    def encode_etc2_rgba(self, blocks, options=None, out=None, stream=None, compression_data=None):
        """Batched cvtt::Kernels::EncodeETC2RGBA: (N,16,4) uint8 -> (N,16) uint8 = [EAC alpha | colour]."""
        return self.encode("etc2rgba", blocks, options, None, out, stream, compression_data)

    def encode_etc2_alpha(self, blocks, options=None, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeETC2Alpha (EAC 8-bit): (N,16,4) uint8 -> (N,8) uint8."""
        return self.encode("eac", blocks, options, None, out, stream)

    def encode_etc2_alpha11(self, blocks, signed=False, options=None, out=None, stream=None):
        """Batched cvtt::Kernels::EncodeETC2Alpha11 (EAC R11): (N,16) int16 PixelBlockScalarS16 -> (N,8) uint8."""
        return self.encode("r11s" if signed else "r11u", blocks, options, None, out, stream)

    # -- decoders (cvtt::Kernels::DecodeBC7 / DecodeBC6HU / DecodeBC6HS) --
    def decode_bc7(self, packed, stream=None):
        """(N,16) uint8 packed BC7 blocks (numpy or CUDA tensor) -> (N,16,4) uint8 PixelBlockU8"""
        return self.decode("bc7", packed, stream)

    def decode_bc6h(self, packed, signed=False, stream=None):
        """(N,16) uint8 packed BC6H blocks -> (N,16,4) int16 half bit patterns (alpha = 0x3C00)"""
        return self.decode("bc6hs" if signed else "bc6hu", packed, stream)

    def psnr_bc7(self, blocks, packed):
        """PSNR (dB, over the four channels) of the decoded `packed` blocks against the source PixelBlockU8 tensor, on the device"""
        import torch
        d = self.decode_bc7(packed).to(torch.float32) - blocks.reshape(-1, 16, 4).to(torch.float32)
        mse = float((d * d).mean().item())
        return float("inf") if mse == 0.0 else 10.0 * float(np.log10(255.0 * 255.0 / mse))

    # -- every format: decode, and the encoding error in one pass (include/cvtt_mi355x.h) --
    @staticmethod
    def _texture_format(fmt):
        if fmt not in TEXTURE_FORMATS:
            raise CvttError("unknown format %r" % (fmt,))
        return TEXTURE_FORMATS[fmt]

    @staticmethod
    def _decoded_layout(fmt, n):
        """(shape, numpy dtype) of the decoded blocks: what the format's encoder reads"""
        if texel_class(fmt) == "half":
            return (n, 16, 4), np.int16
        if texel_class(fmt) == "r11":
            return (n, 16), np.int16
        return (n, 16, 4), (np.int8 if texel_class(fmt) == "snorm8" else np.uint8)

    def decode(self, fmt, packed, stream=None):
        """(N, bytes) packed blocks of `fmt` (numpy or CUDA tensor) -> the layout its encoder reads: (N,16,4) uint8
        (BC4S / BC5S int8; BC6H int16 half bits), R11 (N,16) int16"""
        fid, bpb, _, _ = self._texture_format(fmt)
        if isinstance(packed, np.ndarray):
            b = np.ascontiguousarray(packed, np.uint8)
            n = b.size // bpb
            if b.size % bpb or n % NumParallelBlocks:
                raise CvttError("packed must hold a multiple of 8 %d-byte blocks" % bpb)
            shape, dt = self._decoded_layout(fmt, n)
            res = np.empty(shape, dt)
            with self._host_lock:
                self._check(self._lib.cvttmi_decode(self._h, fid, res.ctypes.data, b.ctypes.data, n), "decode(%s)" % fmt)
            return res
        import torch
        b = self._device_in(packed, "packed")
        nbytes = b.numel() * b.element_size()
        n = nbytes // bpb
        if nbytes % bpb or n % NumParallelBlocks:
            raise CvttError("packed must hold a multiple of 8 %d-byte blocks" % bpb)
        shape, dt = self._decoded_layout(fmt, n)
        res = torch.empty(shape, dtype={np.int16: torch.int16, np.int8: torch.int8, np.uint8: torch.uint8}[dt], device=b.device)
        stream = self._stream(stream, b.device)
        self._check(self._lib.cvttmi_decode_device(self._h, fid, res.data_ptr(), b.data_ptr(), n, ctypes.c_void_p(stream)),
                    "decode(%s)" % fmt)
        return res

    def measure_error(self, fmt, blocks, packed, per_block=False, stream=None):
        """Error of the packed blocks of `fmt` against their source `blocks` (the encoder's input layout: PixelBlockU8,
        PixelBlockS8 for BC4S / BC5S, PixelBlockF16 for BC6H, PixelBlockScalarS16 for R11), decoded in registers on the
        device.  numpy inputs go through the host entry, CUDA tensors through the device entry on `stream`.
        per_block: also return each block's summed squared error (uint32; float32 for BC6H) as ErrorReport.per_block."""
        fid, bpb, tex, _ = self._texture_format(fmt)
        hdr = texel_class(fmt) == "half"
        if isinstance(packed, np.ndarray):
            b = np.ascontiguousarray(packed, np.uint8)
            s = np.ascontiguousarray(blocks)
            n = b.size // bpb
            if b.size % bpb or n % NumParallelBlocks or s.nbytes != n * tex:
                raise CvttError("packed must hold a multiple of 8 %d-byte blocks and blocks exactly as many %d-byte source blocks"
                                % (bpb, tex))
            totals = ErrorTotals()
            pb = np.empty(n, np.float32 if hdr else np.uint32) if per_block else None
            with self._host_lock:
                self._check(self._lib.cvttmi_measure_error(self._h, fid, b.ctypes.data, s.ctypes.data, n,
                                                           pb.ctypes.data if per_block else None, ctypes.addressof(totals)),
                            "measure_error(%s)" % fmt)
            return ErrorReport(fmt, totals, pb)
        import torch
        b = self._device_in(packed, "packed")
        s = self._device_in(blocks, "blocks")
        nbytes = b.numel() * b.element_size()
        n = nbytes // bpb
        if nbytes % bpb or n % NumParallelBlocks or s.numel() * s.element_size() != n * tex:
            raise CvttError("packed must hold a multiple of 8 %d-byte blocks and blocks exactly as many %d-byte source blocks"
                            % (bpb, tex))
        return self._measure_device(fmt, n, per_block, stream, b.device, lambda pb, tot, st: self._lib.cvttmi_measure_error_device(
            self._h, fid, b.data_ptr(), s.data_ptr(), n, pb, tot, st))

    def _measure_device(self, fmt, n, per_block, stream, device, call):
        import torch
        hdr = texel_class(fmt) == "half"
        # (per-block values are uint32 below 2^31 -- at most 16 x 2047^2 -- so an int32 tensor holds them; the totals need no
        # initial value: the call writes all of them, on `stream`)
        tot = torch.empty(ctypes.sizeof(ErrorTotals), dtype=torch.uint8, device=device)
        pb = torch.empty(n, dtype=torch.float32 if hdr else torch.int32, device=device) if per_block else None
        stream = self._stream(stream, device)
        self._check(call(pb.data_ptr() if per_block else None, tot.data_ptr(), ctypes.c_void_p(stream)), "measure(%s)" % fmt)
        torch.cuda.synchronize(device)
        totals = ErrorTotals.from_buffer_copy(tot.cpu().numpy().tobytes())
        return ErrorReport(fmt, totals, pb)

    def measure_image(self, fmt, image, packed, per_block=False, stream=None):
        """Error of `packed` (what encode_image(fmt, image) returns: ceil(W/4) x ceil(H/4) blocks, row-major) against the
        (H,W,4) CUDA image it was encoded from (uint8 RGBA8; a 2-byte dtype for BC6H's RGBA16F); texels outside W x H count
        nowhere.  Every format but R11."""
        import torch
        fid, bpb, _, _ = self._texture_format(fmt)
        if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dim() == 3 and image.shape[2] == 4):
            raise CvttError("image must be a CUDA tensor of shape (H, W, 4)")
        if image.device.index != self.device:
            raise CvttError("image lives on cuda:%d but this context was created for cuda:%d" % (image.device.index, self.device))
        if image.stride(2) != 1 or image.stride(1) != 4:
            image = image.contiguous()
        h, w = int(image.shape[0]), int(image.shape[1])
        esz = image.element_size()
        b = self._device_in(packed, "packed")
        n = ((w + 3) // 4) * ((h + 3) // 4)
        if b.numel() * b.element_size() != n * bpb:
            raise CvttError("packed must hold the %d blocks of a %dx%d image" % (n, w, h))
        return self._measure_device(fmt, n, per_block, stream, b.device, lambda pb, tot, st: self._lib.cvttmi_measure_image_error_device(
            self._h, fid, b.data_ptr(), image.data_ptr(), w, h, image.stride(0) * esz, 0 if esz == 1 else 1, pb, tot, st))

    def selftest_arith(self, count=1 << 22, seed=1):
        """(divide mismatches, sqrt mismatches) of the device against the host's IEEE results"""
        d, q = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.cvttmi_selftest_arith(self._h, count, seed, ctypes.byref(d), ctypes.byref(q)), "selftest_arith")
        return int(d.value), int(q.value)

    def selftest_mfma_i8(self, a, b):
        """(32, 16) int8 . (16, 32) int8 -> (32, 32) int32 by the matrix-core instruction of the BC7 first-tier sums, with the
        operand maps that kernel relies on (csrc/mfma_i8.h)"""
        a = np.ascontiguousarray(a, dtype=np.int8)
        b = np.ascontiguousarray(b, dtype=np.int8)
        if a.shape != (32, 16) or b.shape != (16, 32):
            raise CvttError("selftest_mfma_i8 takes a (32, 16) and a (16, 32) int8 array")
        out = np.empty((32, 32), np.int32)
        fn = self._lib.cvttmi_selftest_mfma_i8
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        self._check(fn(self._h, a.ctypes.data, b.ctypes.data, out.ctypes.data), "selftest_mfma_i8")
        return out

    def selftest_endpoint_byte(self):
        """(mismatches, lowest mismatching bit pattern or None): the BC7 kernels' two-instruction endpoint byte
        (csrc/cvtt_kernel_common.h, endpointByte) against (int)clampRound(x, 255) on all 2^32 binary32 bit patterns"""
        fn = self._lib.cvttmi_selftest_endpoint_byte
        fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
        n, first = ctypes.c_uint64(0), ctypes.c_uint32(0)
        self._check(fn(self._h, ctypes.byref(n), ctypes.byref(first)), "selftest_endpoint_byte")
        return int(n.value), (int(first.value) if n.value else None)

    # -- image -> PixelBlock tiling on the device (reference etc2packer.cpp:215-247, 275-281) --
    def tile_image(self, image, stream=None):
        """(H,W,4) CUDA tensor, uint8 (RGBA8) or a 2-byte dtype (RGBA16F bit patterns), rows may be
        strided -> (ceil(H/4) * ceil(ceil(W/4)/8)*8, 16, 4) PixelBlock tensor: groups of eight
        horizontally adjacent blocks, reads clamped at the right / bottom edge."""
        import torch
        image = self._image_in(image)
        h, w = int(image.shape[0]), int(image.shape[1])
        esz = image.element_size()
        n = self._lib.cvttmi_tiled_block_count(w, h)
        blocks = torch.empty((n, 16, 4), dtype=image.dtype, device=image.device)
        if stream is None:
            stream = torch.cuda.current_stream(image.device).cuda_stream
        self._check(self._lib.cvttmi_tile_image_device(self._h, blocks.data_ptr(), image.data_ptr(), w, h,
                                                       image.stride(0) * esz, 0 if esz == 1 else 1, ctypes.c_void_p(stream)), "tile_image")
        return blocks

    def compact_rows(self, packed, width, height, stream=None):
        """drop the blocks that only pad the last group of every block row: (padded N, B) -> (ceil(H/4)*ceil(W/4), B)"""
        import torch
        packed = self._device_in(packed, "packed")
        bpb = int(packed.shape[1])
        out = torch.empty((((height + 3) // 4) * ((width + 3) // 4), bpb), dtype=torch.uint8, device=packed.device)
        if stream is None:
            stream = torch.cuda.current_stream(packed.device).cuda_stream
        self._check(self._lib.cvttmi_compact_rows_device(self._h, out.data_ptr(), packed.contiguous().data_ptr(), width, height, bpb,
                                                         ctypes.c_void_p(stream)), "compact_rows")
        return out

    def encode_image(self, fmt, image, options=None, plan=None, stream=None):
        """linear image in HBM -> packed blocks of format `fmt`, row-major, ceil(W/4) blocks per row: tiling, encode and
        row compaction all on the device.  fmt: "bc7", "bc1", "bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s", "etc1",
        "etc2" (= "etc2rgb"), "etc2rgba", "etc2punchthrough", "eac" (8-bit EAC alpha block alone) from an (H,W,4) uint8 image;
        "bc6hu", "bc6hs" from an (H,W,4) half-float image."""
        h, w = int(image.shape[0]), int(image.shape[1])
        blocks = self.tile_image(image, stream)
        if not has_image_form(fmt):  # (R11 reads PixelBlockScalarS16: no image form)
            raise CvttError("unknown format %r" % (fmt,))
        packed = self.encode(fmt, blocks, options, plan, stream=stream)
        return packed if w % 32 == 0 else self.compact_rows(packed, w, h, stream)

    def _image_in(self, image):
        """the (H, W, 4) image of tile_image / build_mips, texels contiguous (rows may be strided)"""
        import torch
        if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dim() == 3 and image.shape[2] == 4):
            raise CvttError("image must be a CUDA tensor of shape (H, W, 4)")
        if image.device.index != self.device:
            raise CvttError("image lives on cuda:%d but this context was created for cuda:%d" % (image.device.index, self.device))
        if image.element_size() not in (1, 2):
            raise CvttError("image must be RGBA8 or RGBA16F")
        return image if image.stride(2) == 1 and image.stride(1) == 4 else image.contiguous()

    def _one_layer(self, image):
        """the (H, W, 4) image of build_mips / encode_mips as a (1, H, W, 4) view, never a copy of its rows: a row stride the
        single-image C entry refuses (below the row, or no whole texels) is refused here as it was there"""
        image = self._image_in(image)
        if image.stride(0) < 4 * image.shape[1] or image.stride(0) % 4:
            raise CvttError("image rows must be whole texels and at least a row apart")
        return image[None]

    # -- mip chains: 2x2 filter on the device, and the whole chain through one encode call --
    def build_mips(self, image, levels=None, signed=False, stream=None, filter="box", kernel=None, wrap="clamp", hdr=None):
        """(H,W,4) CUDA image -> the list of its mip levels (build_mips_array of one layer): [0] is the image itself, the others are
        (h_L, w_L, 4) views of the image's dtype into ONE allocation laid out by mip_layout.  Level L+1 is max(1, w_L >> 1) x
        max(1, h_L >> 1), a 2x2 box of the rounded level L (an odd last row / column is dropped).  uint8: (a+b+c+d+2) >> 2;
        int8, or signed=True (the bytes BC4S / BC5S read): the same on int8 with an arithmetic shift; a 2-byte dtype: RGBA16F,
        ((a+b)+(c+d)) * 0.25 in float, rounded to nearest even.  levels: None = the full chain down to 1x1.
        filter (cvttmi_build_mips_filtered_device; a name or a MIP_FILTER_* value): "box" is the rule above; "srgb" averages the
        colour channels of a uint8 image in linear light; "box+alpha" / "srgb+alpha" weight them by the texels' alphas; "normal"
        renormalises the summed vectors of a uint8 or int8 normal map.  Alpha always takes the box rule.
        kernel: None = the 2x2 rules above; "triangle", "mitchell", "lanczos3" or "kaiser" (MIP_KERNELS) filters every level with
        that kernel's 4 / 8 / 12 taps per direction instead, under "box" (the plain rule), "srgb" or "normal", uint8 or int8
        images; an odd last row / column is then read as a neighbour.  wrap: how the taps leave the image: "clamp", "repeat" (a
        tiling texture) or "mirror"; only with a kernel.
        hdr: the range of an RGBA16F image under a kernel, "nonnegative" (results clamped to [+0, 65504]) or "signed" ([-65504,
        65504]) -- a kernel with negative lobes rings below zero in HDR data.  Such an image takes a kernel with the "box" rule and
        a range only: the sums in float32, every product and sum rounded on its own (cvtt_mi355x.h).  None: a half image under a
        kernel is a CvttError; a range with anything else is one too."""
        return self.build_mips_array(self._one_layer(image), levels, signed, stream, filter, kernel, wrap, hdr)[0]

    def encode_mips(self, fmt, image, options=None, plan=None, levels=None, stream=None, mip_filter="box", kernel=None, wrap="clamp",
                    hdr=None):
        """(H,W,4) CUDA image -> the packed blocks of every mip level: a list of (ceil(w_L/4) * ceil(h_L/4), bytes per block)
        uint8 views, level 0 first, consecutive in one allocation (container order): encode_texture of one layer.  Level L equals
        encode_image(fmt, build_mips(image)[L]) byte for byte; the levels are tiled into one block tensor and searched by ONE
        encode call (groups of eight blocks are independent), so the small levels cost no launches of their own.  fmt as for
        encode_image; "bc4s" / "bc5s" average the image as int8.  levels: None = the full chain.  mip_filter: build_mips's
        `filter`, under which "Level L equals ..." reads encode_image(fmt, build_mips(image, filter=mip_filter)[L]); kernel, wrap,
        hdr: build_mips's, and the same holds under them ("bc6hu" / "bc6hs" with a kernel need hdr).
        The averaging rule follows the format, so an int8 image is taken by "bc4s" / "bc5s" alone: with any other format it is a
        CvttError (it was one for "bc7" before; the other formats used to average it as int8 and encode the bytes).
        The levels are views of the allocation that also holds the call's work space (pyramids, tiles, padded blocks: several
        times the blocks' size), so that kernels on a caller's own stream never outlive it: any level kept keeps all of it.
        Copy (clone) the levels to keep for long."""
        import torch
        if not has_image_form(fmt):  # (R11 reads PixelBlockScalarS16: no image form)
            raise CvttError("unknown format %r" % (fmt,))
        if isinstance(image, torch.Tensor) and image.dtype == torch.int8 and texel_class(fmt) != "snorm8":
            raise CvttError("%s is not encoded from an int8 image (bc4s / bc5s are)" % fmt)
        return self.encode_texture(fmt, self._one_layer(image), options, plan, levels, "layer", mip_filter, stream, kernel, wrap, hdr)[0]

    # -- texture arrays and cube maps: `layers` images of one size through mips and encode at once (cvtt_mi355x.h) --
    def _images_in(self, images):
        """the (L, H, W, 4) images of build_mips_array / encode_texture, texels contiguous (rows and layers may be strided);
        a list of (H, W, 4) tensors is stacked once -> (tensor, row pitch in bytes, layer pitch in bytes)"""
        import torch
        if isinstance(images, (list, tuple)):
            images = [self._image_in(t) for t in images]
            if not images or any(t.shape != images[0].shape or t.dtype != images[0].dtype for t in images):
                raise CvttError("images must be a non-empty list of (H, W, 4) tensors of one size and dtype")
            images = torch.stack(images)
        if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dim() == 4 and images.shape[3] == 4 and images.shape[0] >= 1
                and images.shape[1] >= 1 and images.shape[2] >= 1):
            raise CvttError("images must be a CUDA tensor of shape (L, H, W, 4) or a list of (H, W, 4) CUDA tensors")
        if images.device.index != self.device:
            raise CvttError("images live on cuda:%d but this context was created for cuda:%d" % (images.device.index, self.device))
        if images.element_size() not in (1, 2):
            raise CvttError("images must be RGBA8 or RGBA16F")
        n, h, w = (int(v) for v in images.shape[:3])
        # a stride of a dimension of size 1 says nothing: such a pitch is the tight one
        row = images.stride(1) if h > 1 else 4 * w
        layer = images.stride(0) if n > 1 else h * row
        if not (images.stride(3) == 1 and images.stride(2) == 4 and row >= 4 * w and row % 4 == 0 and layer >= h * row and layer % 4 == 0):
            images = images.contiguous()
            row, layer = 4 * w, 4 * w * h
        esz = images.element_size()
        return images, row * esz, layer * esz

    @staticmethod
    def _pixel_kind(images, signed):
        """the PIXELS_* kind of _images_in's tensor: float16 is RGBA16F, int8 or signed=True the int8 reading of RGBA8"""
        import torch
        return PIXELS_RGBA16F if images.element_size() == 2 else PIXELS_RGBA8_SNORM if (signed or images.dtype == torch.int8) else PIXELS_RGBA8

    def build_mips_array(self, images, levels=None, signed=False, stream=None, filter="box", kernel=None, wrap="clamp", hdr=None):
        """(L, H, W, 4) CUDA tensor (or a list of (H, W, 4) ones) -> [layer][level] images (cvttmi_build_mips_array_device): the mip
        chain of every layer, ONE launch per level for all of them.  [l][0] is a view of the input, the others are (h_L, w_L, 4) views
        into one allocation: layer l's chain as mip_layout places it, texture_layout's pyramidLayerBytes apart.  levels, signed,
        filter, kernel, wrap, hdr: as for build_mips."""
        import torch
        images, row_pitch, layer_pitch = self._images_in(images)
        n, h, w = (int(v) for v in images.shape[:3])
        esz = images.element_size()
        if esz == 2 and signed:
            raise CvttError("signed selects the int8 rule of an RGBA8 image")
        kind = self._pixel_kind(images, signed)
        layout = mip_layout(w, h, 4 * esz, 16, levels)
        sizes = texture_layout(w, h, 4 * esz, 16, len(layout), n)
        pyramids = torch.empty(sizes.pyramidBytes, dtype=torch.uint8, device=images.device)
        self._check(self._lib.cvttmi_build_mips_array_device(self._h, pyramids.data_ptr(), sizes.pyramidBytes, images.data_ptr(), w, h, row_pitch,
                                                             layer_pitch, kind, len(layout), n, mip_filter_word(filter, kernel, wrap, hdr),
                                                             ctypes.c_void_p(self._stream(stream, images.device))), "build_mips_array")
        # one strided view per level over all layers, then its n slices (pyramidLayerBytes is a multiple of 256: whole elements)
        typed = pyramids.view(images.dtype)
        per_level = [images.unbind(0)] + [typed.as_strided((n, L.height, L.width, 4), (sizes.pyramidLayerBytes // esz, 4 * L.width, 4, 1),
                                                           L.byteOffset // esz).unbind(0) for L in layout[1:]]
        return [[views[l] for views in per_level] for l in range(n)]

    # -- resize: any size to any size on the device (cvtt_mi355x.h, "resize") --
    def resize(self, images, width, height, kernel="lanczos3", filter="box", wrap="clamp", signed=False, out=None, stream=None, hdr=None):
        """(H, W, 4) or (L, H, W, 4) CUDA tensor, uint8 or int8 (float16 with hdr) -> the same rank resized to `width` x `height`
        (cvttmi_resize_image_device: all layers in one call).  kernel: "box" (area average), "triangle", "mitchell", "lanczos3" or
        "kaiser"; going down it is stretched by the ratio, going up it is not.  filter: "box" (the plain rule), "srgb" (colour in
        linear light, uint8 only) or "normal" (renormalised) -- build_mips's names without the "+alpha" ones; wrap: "clamp",
        "repeat" or "mirror".  int8, or signed=True: the bytes are read as int8.  At exactly half the size the result is
        build_mips(kernel=kernel)[1].  out: a CUDA tensor of the result's shape and dtype to write into (its rows and layers may be
        strided, its texels not).
        hdr: "nonnegative" or "signed" (MIP_HDR) = the images are float16 (RGBA16F), resized under the "box" rule in float32 with the
        results clamped to [+0, 65504] or [-65504, 65504] (build_mips's hdr; here it goes with every kernel, "box" included).  None: a
        float16 image is a CvttError."""
        import torch
        single = isinstance(images, torch.Tensor) and images.dim() == 3
        images, row_pitch, layer_pitch = self._images_in(self._one_layer(images) if single else images)
        if hdr is None and images.element_size() != 1:
            raise CvttError("resize takes RGBA8 images (uint8 or int8), and float16 images with hdr=")
        if hdr is not None and images.dtype != torch.float16:
            raise CvttError("hdr= goes with float16 images")
        if hdr is not None and signed:
            raise CvttError("signed selects the int8 rule of an RGBA8 image")
        esz = images.element_size()
        n, h, w = (int(v) for v in images.shape[:3])
        width, height = _u32(width, "width"), _u32(height, "height")
        kind = self._pixel_kind(images, signed)
        word = resize_filter_word(kernel, filter, wrap, hdr)
        shape = (n, height, width, 4)
        if out is None:
            result = torch.empty(shape, dtype=images.dtype, device=images.device)
        else:
            result = out[None] if (isinstance(out, torch.Tensor) and out.dim() == 3) else out
            if not (isinstance(result, torch.Tensor) and result.is_cuda and result.device == images.device and tuple(result.shape) == shape
                    and result.dtype == images.dtype):
                raise CvttError("out must be a CUDA tensor on %s of shape %s and dtype %s" % (images.device, shape[1:] if single else shape, images.dtype))
            kept, out_row, out_layer = self._images_in(result)
            if kept is not result:
                raise CvttError("out must have contiguous texels, rows at least a row apart and layers at least an image apart")
        if out is None:
            out_row, out_layer = 4 * width * esz, 4 * width * height * esz
        need = ctypes.c_size_t(0)
        rc = self._lib.cvttmi_resize_work_bytes(w, h, width, height, kind, word, n, ctypes.byref(need))
        if rc != 0:
            raise CvttError("resize %dx%d -> %dx%d refused: sizes and layers are 1 .. 65535; uint8 images take box, srgb and normal, int8 images box "
                            "and normal, float16 images box with hdr=" % (w, h, width, height))
        work = torch.empty(max(need.value, 1), dtype=torch.uint8, device=images.device)
        self._check(self._lib.cvttmi_resize_image_device(self._h, result.data_ptr(), width, height, out_row, out_layer, images.data_ptr(), w, h,
                                                         row_pitch, layer_pitch, kind, n, word, work.data_ptr(), need.value,
                                                         ctypes.c_void_p(self._stream(stream, images.device))), "resize")
        if stream is not None:  # the work space is read on the caller's stream: the allocator must not hand it out before that
            work.record_stream(torch.cuda.ExternalStream(stream, device=images.device))
        return out if out is not None else (result[0] if single else result)

    def encode_texture(self, fmt, images, options=None, plan=None, levels=None, order="layer", mip_filter="box", stream=None, kernel=None,
                       wrap="clamp", hdr=None):
        """(L, H, W, 4) CUDA tensor (or a list of (H, W, 4) ones): the layers of a texture array, or the 6 n faces of a cube (array)
        in the order +X -X +Y -Y +Z -Z -> TextureBlocks: [layer][level] packed blocks, uint8 views into ONE allocation (.base) in
        `order`: "layer" = every layer's chain consecutive (DDS), "level" = every level's layers consecutive (KTX).  One C call
        (cvttmi_encode_texture_device): the mips of all layers a launch per level, one tile launch, one search, one compact launch.
        [l][L] equals encode_image(fmt, build_mips_array(images, ..)[l][L]) byte for byte.  fmt, levels, mip_filter, kernel, wrap, hdr:
        as for encode_mips.  The allocation behind .base also holds the call's work space (texture_layout's workBytes, several times the
        blocks), so any view kept keeps that too: clone what is kept for long."""
        import torch
        if not has_image_form(fmt):  # (R11 reads PixelBlockScalarS16: no image form)
            raise CvttError("unknown format %r" % (fmt,))
        fid, bpb, _, _ = TEXTURE_FORMATS[fmt]
        images, row_pitch, layer_pitch = self._images_in(images)
        n, h, w = (int(v) for v in images.shape[:3])
        esz = images.element_size()
        if (esz == 2) != (texel_class(fmt) == "half"):
            raise CvttError("%s is encoded from %s images" % (fmt, "RGBA16F" if esz == 1 else "RGBA8"))
        options = options if options is not None else Options()
        if fmt == "bc7" and plan is None:
            plan = BC7EncodingPlan()
        levels = mip_level_count(w, h) if levels is None else int(levels)
        ov = order_value(order)
        sizes = texture_layout(w, h, 4 * esz, bpb, levels, n, ov)
        # blocks and work space in one allocation: every view of the blocks (.base among them) keeps the work space alive, which the
        # kernels of a caller's own stream may still be using
        out_bytes = sizes.blocks * bpb
        both = torch.empty(-(-out_bytes // 256) * 256 + sizes.workBytes, dtype=torch.uint8, device=images.device)
        out, work = both[:out_bytes].view(sizes.blocks, bpb), both[both.numel() - sizes.workBytes:]
        self._check(self._lib.cvttmi_encode_texture_device(self._h, fid, out.data_ptr(), sizes.blocks * bpb, images.data_ptr(), w, h, row_pitch,
                                                           layer_pitch, n, levels, mip_filter_word(mip_filter, kernel, wrap, hdr), ov,
                                                           ctypes.addressof(options),
                                                           ctypes.addressof(plan) if plan is not None else None, None, work.data_ptr(),
                                                           sizes.workBytes, ctypes.c_void_p(self._stream(stream, images.device))),
                    "encode_texture(%s)" % fmt)
        res = TextureBlocks()
        res.base, res.order = out, "level" if ov == ORDER_LEVEL_MAJOR else "layer"
        # one strided view per level over all layers, then its n slices: a few tensor operations per level, not per subresource
        per_level = [out.as_strided((n, count, bpb), (step * bpb, bpb, 1), first * bpb).unbind(0)
                     for first, step, count in _texture_places(w, h, 4 * esz, bpb, levels, n, ov)]
        res.extend([views[l] for views in per_level] for l in range(n))
        return res


    # -- packed blocks -> linear images on the device (cvtt_mi355x.h, "decoding into images") --
    @staticmethod
    def _image_dtype(fmt):
        """torch dtype of the (H, W, 4) image `fmt` decodes into"""
        import torch
        return torch.float16 if texel_class(fmt) == "half" else torch.int8 if texel_class(fmt) == "snorm8" else torch.uint8

    def _image_format(self, fmt, what):
        if not has_image_form(fmt):  # (R11 decodes to PixelBlockScalarS16: no image form)
            raise CvttError("%s: %r has no image form" % (what, fmt) if fmt in TEXTURE_FORMATS else "unknown format %r" % (fmt,))
        return TEXTURE_FORMATS[fmt][:2]

    def _packed_in(self, packed, nbytes, what):
        """a CUDA tensor of this context's device holding exactly `nbytes`"""
        import torch
        if not (isinstance(packed, torch.Tensor) and packed.is_cuda):
            raise CvttError("%s must be a CUDA tensor" % what)
        if packed.device.index != self.device:
            raise CvttError("%s lives on cuda:%d but this context was created for cuda:%d" % (what, packed.device.index, self.device))
        if packed.numel() * packed.element_size() != nbytes:
            raise CvttError("%s must hold exactly %d bytes, got %d" % (what, nbytes, packed.numel() * packed.element_size()))
        return packed.contiguous()

    def decode_image(self, fmt, packed, width, height, out=None, stream=None):
        """The ceil(W/4) x ceil(H/4) packed blocks of `fmt` (a CUDA tensor: what encode_image returns and a container holds;
        any count) -> the (H, W, 4) CUDA image: uint8, int8 for bc4s / bc5s, float16 for BC6H, texel values as decode() gives
        them.  Every format but R11.  out: an (H, W, 4) CUDA tensor of that dtype to decode into, texels contiguous
        (stride(2) == 1, stride(1) == 4), any row stride of at least 4 * W elements -- a window of an atlas; only the texels of
        the image are written, and `out` is never replaced by a copy."""
        import torch
        fid, bpb = self._image_format(fmt, "decode_image")
        w, h = int(width), int(height)
        if w < 1 or h < 1:
            raise CvttError("decode_image: a %d x %d image" % (w, h))
        b = self._packed_in(packed, ((w + 3) // 4) * ((h + 3) // 4) * bpb, "packed (the blocks of a %dx%d %s image)" % (w, h, fmt))
        dtype = self._image_dtype(fmt)
        if out is None:
            out = torch.empty((h, w, 4), dtype=dtype, device=b.device)
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == b.device and out.dtype == dtype
                  and tuple(out.shape) == (h, w, 4) and out.stride(2) == 1 and out.stride(1) == 4
                  and (h == 1 or (out.stride(0) >= 4 * w and out.stride(0) % 4 == 0)) and out.data_ptr() % (4 * out.element_size()) == 0):
            raise CvttError("out must be a (%d, %d, 4) %s CUDA tensor on %s with contiguous texels and a row stride of whole texels, "
                            "at least %d elements" % (h, w, str(dtype).replace("torch.", ""), b.device, 4 * w))
        esz = out.element_size()
        pitch = (out.stride(0) if h > 1 else 4 * w) * esz
        self._check(self._lib.cvttmi_decode_image_device(self._h, fid, out.data_ptr(), pitch, PIXELS_RGBA16F if esz == 2 else PIXELS_RGBA8,
                                                         b.data_ptr(), w, h, ctypes.c_void_p(self._stream(stream, b.device))),
                    "decode_image(%s)" % fmt)
        return out

    def decode_mips(self, fmt, levels, width, height, stream=None):
        """[packed blocks of level L] of a width x height texture (CUDA tensors: what encode_mips returns, or the levels
        read_ktx_mips / read_dds_mips give, uploaded) -> the list of the decoded levels (cvttmi_decode_mips_device, ONE launch
        for the chain): [0] an (H, W, 4) tensor of its own, the others (h_L, w_L, 4) views into one allocation laid out by
        mip_layout, like build_mips.  Levels that are not already consecutive in one allocation are concatenated once."""
        import torch
        fid, bpb = self._image_format(fmt, "decode_mips")
        levels = list(levels)
        w, h = int(width), int(height)
        if w < 1 or h < 1 or not 1 <= len(levels) <= max(w, h).bit_length():
            raise CvttError("decode_mips: a %d x %d texture has 1 .. %d levels, got %d" % (w, h, max(w, h, 1).bit_length(), len(levels)))
        dtype = self._image_dtype(fmt)
        esz = 2 if dtype == torch.float16 else 1
        layout = mip_layout(w, h, 4 * esz, bpb, len(levels))
        levels = [self._packed_in(t, L.blockCount * bpb, "level %d (the blocks of a %dx%d %s image)" % (l, L.width, L.height, fmt))
                  for l, (t, L) in enumerate(zip(levels, layout))]
        base = levels[0].data_ptr()
        if all(t.data_ptr() == base + L.packedByteOffset for t, L in zip(levels, layout)):
            packed = levels[0]  # (already in container order, as encode_mips returns them)
        else:
            packed = torch.cat([t.reshape(-1).view(torch.uint8) for t in levels])
        image = torch.empty((h, w, 4), dtype=dtype, device=packed.device)
        pyramid = torch.empty(layout.pyramid_bytes, dtype=torch.uint8, device=packed.device)
        self._check(self._lib.cvttmi_decode_mips_device(self._h, fid, image.data_ptr(), 4 * w * esz, pyramid.data_ptr() if len(layout) > 1 else None,
                                                        layout.pyramid_bytes, PIXELS_RGBA16F if esz == 2 else PIXELS_RGBA8, packed.data_ptr(),
                                                        w, h, len(layout), ctypes.c_void_p(self._stream(stream, packed.device))),
                    "decode_mips(%s)" % fmt)
        return [image] + [pyramid[L.byteOffset: L.byteOffset + L.rowPitchBytes * L.height].view(dtype).view(L.height, L.width, 4)
                          for L in layout[1:]]


_default_ctx = {}


def shard_block_rows(block_rows, blocks_per_row, rank, world):
    """cvttmi_shard_block_rows: [first, last) of `rank`'s shard -- whole block rows, group aligned (the C statement of
    sharding.shard_block_rows; needs no device)"""
    lib = load_library()
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    rc = lib.cvttmi_shard_block_rows(block_rows, blocks_per_row, rank, world, ctypes.byref(lo), ctypes.byref(hi))
    if rc != 0:
        raise CvttError("cvttmi_shard_block_rows failed (%d)" % rc)
    return lo.value, hi.value


class MultiContext:
    """One job on several devices behind the C ABI (cvttmi_multi_*, csrc/multi.cpp): one context per entry of `devices` (a
    device may appear more than once), block-row shards, packed output straight into the caller's buffer.  Host arrays only.
    Every format with an encoder: the names of TEXTURE_FORMATS."""
    FORMATS = {name: (fid, tex, bpb) for name, (fid, bpb, tex, _) in TEXTURE_FORMATS.items()}  # name -> (id, in bytes, out bytes)

    def __init__(self, devices):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        self.devices = [int(d) for d in devices]
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        rc = self._lib.cvttmi_multi_create(ctypes.byref(self._h), arr, len(self.devices))
        if rc != 0:
            raise CvttError("cvttmi_multi_create(%s) failed with %d" % (self.devices, rc))

    def close(self):
        if self._h:
            self._lib.cvttmi_multi_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_rcp_table(self, lut):
        lut = np.ascontiguousarray(lut, np.float32)
        assert lut.size == 17
        rc = self._lib.cvttmi_multi_set_rcp_table(self._h, lut.ctypes.data)
        if rc != 0:
            raise CvttError("cvttmi_multi_set_rcp_table failed (%d)" % rc)

    def set_exhaustive(self, on=True):
        self._lib.cvttmi_multi_set_exhaustive(self._h, 1 if on else 0)

    def last_shards(self):
        out = []
        for i in range(len(self.devices)):
            lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
            self._lib.cvttmi_multi_last_shard(self._h, i, ctypes.byref(lo), ctypes.byref(hi))
            out.append((lo.value, hi.value))
        return out

    def encode(self, fmt, blocks, options=None, plan=None, blocks_per_row=0, out=None):
        code, in_bytes, out_bytes = self.FORMATS[fmt]
        options = options if options is not None else Options()
        if fmt == "bc7" and plan is None:
            plan = BC7EncodingPlan()
        b = np.ascontiguousarray(blocks)
        n = b.nbytes // in_bytes
        if b.nbytes % in_bytes or n % NumParallelBlocks:
            raise CvttError("blocks must hold a multiple of 8 PixelBlocks")
        res = out if out is not None else np.empty((n, out_bytes), np.uint8)
        assert res.nbytes == n * out_bytes and res.flags["C_CONTIGUOUS"]
        rc = self._lib.cvttmi_multi_encode(self._h, code, res.ctypes.data, b.ctypes.data, n, blocks_per_row,
                                           ctypes.addressof(options), ctypes.addressof(plan) if plan is not None else None)
        if rc != 0:
            raise CvttError("cvttmi_multi_encode(%s) failed (%d): %s" % (fmt, rc, self._lib.cvttmi_multi_last_error(self._h).decode()))
        return res


    def encode_device(self, fmt, shards, out, blocks_per_row=0, options=None, plan=None):
        """cvttmi_multi_encode_device: `shards[r]` = a device tensor on devices[r] holding shard r's PixelBlocks (None for an empty
        shard), `out` = a device tensor on devices[0] for all the packed blocks.  The shard table is that of
        shard_block_rows(rows, blocks_per_row, r, len(devices)); returns `out` when it is complete."""
        code, in_bytes, out_bytes = self.FORMATS[fmt]
        options = options if options is not None else Options()
        if fmt == "bc7" and plan is None:
            plan = BC7EncodingPlan()
        n = out.numel() * out.element_size() // out_bytes
        if len(shards) != len(self.devices):
            raise CvttError("one shard (or None) per device")
        ptrs = (ctypes.c_void_p * len(shards))(*[None if t is None else t.data_ptr() for t in shards])
        import torch
        for t in shards:
            if t is not None:
                torch.cuda.current_stream(t.device).synchronize()  # the library launches on streams of its own
        rc = self._lib.cvttmi_multi_encode_device(self._h, code, out.data_ptr(), ptrs, n, blocks_per_row,
                                                  ctypes.addressof(options), ctypes.addressof(plan) if plan is not None else None)
        if rc != 0:
            raise CvttError("cvttmi_multi_encode_device(%s) failed (%d): %s" % (fmt, rc, self._lib.cvttmi_multi_last_error(self._h).decode()))
        return out


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


# ---- cvtt::Kernels-style free functions (8-block call convention of the reference) ----
def ConfigureBC7EncodingPlanFromQuality(encodingPlan, quality):
    """cvtt::Kernels::ConfigureBC7EncodingPlanFromQuality (BC67.cpp:3291-3352): fills `encodingPlan` in place for quality
    1..100 (clamped).  Host-side; needs no device."""
    if load_library().cvttmi_bc7_plan_from_quality(ctypes.byref(encodingPlan), int(quality)) != 0:
        raise CvttError("cvttmi_bc7_plan_from_quality failed")
    return encodingPlan


def ConfigureBC7EncodingPlanFromFineTuningParams(encodingPlan, params):
    """cvtt::Kernels::ConfigureBC7EncodingPlanFromFineTuningParams (BC67.cpp:3355-3483); returns True like the reference."""
    if load_library().cvttmi_bc7_plan_from_fine_tuning(ctypes.byref(encodingPlan), ctypes.byref(params)) != 0:
        raise CvttError("cvttmi_bc7_plan_from_fine_tuning failed")
    return True


def EncodeBC7(pBlocks, options=None, encodingPlan=None, device=0):
    """cvtt::Kernels::EncodeBC7 (reference ConvectionKernels_API.cpp:41-54): any multiple of
    NumParallelBlocks blocks; returns the packed 16-byte blocks."""
    return default_context(device).encode_bc7(pBlocks, options, encodingPlan)


def EncodeBC2(pBlocks, options=None, device=0):
    """cvtt::Kernels::EncodeBC2 (reference ConvectionKernels_API.cpp:101-115)."""
    return default_context(device).encode_bc2(pBlocks, options)


def EncodeBC3(pBlocks, options=None, device=0):
    return default_context(device).encode_bc3(pBlocks, options)


def EncodeBC4U(pBlocks, options=None, device=0):
    return default_context(device).encode_bc4(pBlocks, options, signed=False)


def EncodeBC4S(pBlocks, options=None, device=0):
    return default_context(device).encode_bc4(pBlocks, options, signed=True)


def EncodeBC5U(pBlocks, options=None, device=0):
    return default_context(device).encode_bc5(pBlocks, options, signed=False)


def EncodeBC5S(pBlocks, options=None, device=0):
    return default_context(device).encode_bc5(pBlocks, options, signed=True)


def EncodeETC2Alpha11(pBlocks, isSigned=False, options=None, device=0):
    """cvtt::Kernels::EncodeETC2Alpha11 (reference ConvectionKernels_API.cpp:258-268)."""
    return default_context(device).encode_etc2_alpha11(pBlocks, isSigned, options)


def DecodeBC7(pBC, device=0):
    """cvtt::Kernels::DecodeBC7 (reference ConvectionKernels_API.cpp:305-310), batched"""
    return default_context(device).decode_bc7(pBC)


def DecodeBC6HU(pBC, device=0):
    return default_context(device).decode_bc6h(pBC, signed=False)


def DecodeBC6HS(pBC, device=0):
    return default_context(device).decode_bc6h(pBC, signed=True)


def EncodeBC1(pBlocks, options=None, device=0):
    """cvtt::Kernels::EncodeBC1 (reference ConvectionKernels_API.cpp:86-99)."""
    return default_context(device).encode_bc1(pBlocks, options)


def EncodeBC6HU(pBlocks, options=None, device=0):
    """cvtt::Kernels::EncodeBC6HU (reference ConvectionKernels_API.cpp:56-69)."""
    return default_context(device).encode_bc6h(pBlocks, options, signed=False)


def EncodeBC6HS(pBlocks, options=None, device=0):
    """cvtt::Kernels::EncodeBC6HS (reference ConvectionKernels_API.cpp:71-84)."""
    return default_context(device).encode_bc6h(pBlocks, options, signed=True)


def EncodeETC1(pBlocks, options=None, compressionData=None, device=0):
    """cvtt::Kernels::EncodeETC1 (reference ConvectionKernels_API.cpp:201-214); the ETC1CompressionData scratch
    argument is accepted and ignored."""
    return default_context(device).encode_etc1(pBlocks, options)


class ETC2CompressionData:
    """What cvtt::Kernels::AllocETC2Data returns (reference ConvectionKernels_ETC.cpp:3100-3145).  The 136 KB of scratch have
    no counterpart (the kernels' scratch is LDS); what the reference fixes at allocation time and the encoder needs later are
    the two chroma axes, derived from the colour weights of the Options given here."""

    def __init__(self, options=None):
        self.alloc_options = Options.frombytes(bytes(options if options is not None else Options()))


def AllocETC2Data(options=None):
    """cvtt::Kernels::AllocETC2Data (no allocator callbacks: nothing is allocated in caller memory)."""
    return ETC2CompressionData(options)


def ReleaseETC2Data(compressionData):
    """cvtt::Kernels::ReleaseETC2Data: nothing to free."""
    return None


def EncodeETC2(pBlocks, options=None, compressionData=None, device=0):
    """cvtt::Kernels::EncodeETC2 (reference ConvectionKernels_API.cpp:216-229).  compressionData: from AllocETC2Data; its
    Options fix the chroma axes, as in the reference (scratch itself lives in LDS)."""
    return default_context(device).encode_etc2(pBlocks, options, compression_data=compressionData)


def EncodeETC2PunchthroughAlpha(pBlocks, options=None, compressionData=None, device=0):
    """cvtt::Kernels::EncodeETC2PunchthroughAlpha (reference ConvectionKernels_API.cpp:231-244)."""
    return default_context(device).encode_etc2_punchthrough_alpha(pBlocks, options, compression_data=compressionData)


def EncodeETC2RGBA(pBlocks, options=None, compressionData=None, device=0):
    """cvtt::Kernels::EncodeETC2RGBA (reference ConvectionKernels_API.cpp:270-286)."""
    return default_context(device).encode_etc2_rgba(pBlocks, options, compression_data=compressionData)


def EncodeETC2Alpha(pBlocks, options=None, device=0):
    """cvtt::Kernels::EncodeETC2Alpha (reference ConvectionKernels_API.cpp:246-256)."""
    return default_context(device).encode_etc2_alpha(pBlocks, options)
