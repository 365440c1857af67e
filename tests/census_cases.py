"""The directed cases of tests/test_mode_census.py and of tests/golden/mode_census.npz (test helper): content from
tests/content.py paired with the Options / BC7EncodingPlan that make the reference emit every encoding of a format.
Everything is regenerated from seeds; a case is (name, kind, blocks, options bytes, plan bytes or None) where `kind` names the
encoder (`encode_oracle`, `encode_reference`, `encode_gpu`)."""
import functools

import numpy as np

import content
from convectionkernels_amd import api
from oracle import pyref

FULL = 0xFFFFFFFFFFFFFFFF


def _bytes(s):
    return np.frombuffer(s.tobytes(), np.uint8).copy()


def single_mode_plan(mode):
    """a BC7EncodingPlan with every other mode off: partition masks 0, mode 6 off, no mode-4 / mode-5 seed points"""
    p = api.BC7EncodingPlan()
    p.mode0PartitionEnabled = 0
    p.mode1PartitionEnabled = p.mode2PartitionEnabled = p.mode3PartitionEnabled = 0
    p.mode7RGBAPartitionEnabled = p.mode7RGBPartitionEnabled = 0
    p.mode6Enabled = 0
    for r in range(4):
        p.mode4SP[r][0] = p.mode4SP[r][1] = p.mode5SP[r] = 0
    if mode == 0:
        p.mode0PartitionEnabled = 0xFFFF
    elif mode == 1:
        p.mode1PartitionEnabled = FULL
    elif mode == 2:
        p.mode2PartitionEnabled = FULL
    elif mode == 3:
        p.mode3PartitionEnabled = FULL
    elif mode == 4:
        for r in range(4):
            p.mode4SP[r][0] = p.mode4SP[r][1] = 4
    elif mode == 5:
        for r in range(4):
            p.mode5SP[r] = 4
    elif mode == 6:
        p.mode6Enabled = 1
    elif mode == 7:
        p.mode7RGBAPartitionEnabled = p.mode7RGBPartitionEnabled = FULL
    else:
        raise ValueError(mode)
    return p


def bc7_options():
    return {"default": api.Options(), "better": api.Options(flags=api.Flags.Better),
            "uniform": api.Options(flags=api.Flags.Default | api.Flags.Uniform)}


# key -> (steered mode, content).  "7a": mode 7 from alpha content, "7o": from opaque content; "4", "5", "6": dual-plane content
@functools.lru_cache(maxsize=None)
def bc7_sets():
    dual = content.dual_plane_blocks(7045)
    return {
        "0": (0, content.partition_shaped_blocks(3, False, 7000)[:128]),
        "1": (1, content.partition_shaped_blocks(2, False, 7001)),
        "2": (2, content.partition_shaped_blocks(3, False, 7002)),
        "3": (3, content.partition_shaped_blocks(2, False, 7003)),
        "7a": (7, content.partition_shaped_blocks(2, True, 7007)),
        "7o": (7, content.partition_shaped_blocks(2, False, 7008)),
        "4": (4, dual), "5": (5, dual), "6": (6, dual),
    }


def bc7_cases(key):
    """the cases of one steered set: its single-mode plan and the default plan x the three option sets"""
    mode, blocks = bc7_sets()[key]
    plans = [("single", single_mode_plan(mode))]
    if key not in ("5", "6"):  # the dual-plane content under the default plan is one case set, not three
        plans.append(("default", api.BC7EncodingPlan()))
    return [("bc7_%s_%s_%s" % (key, pn, on), "bc7", blocks, _bytes(o), _bytes(p))
            for pn, p in plans for on, o in bc7_options().items()]


def bc6h_options():
    return {"default": api.Options(),
            "fast3": api.Options(flags=api.Flags.Default | api.Flags.BC6H_FastIndexing, seedPoints=3),
            "refine1": api.Options(refineRoundsBC6H=1)}


@functools.lru_cache(maxsize=None)
def bc6h_blocks(signed):
    """bc6h_mode_blocks shuffled block by block: the reference couples the eight blocks of a group, and the kernel the lanes
    of a wave, so every group mixes shapes, spreads and emphases"""
    b = content.bc6h_mode_blocks(signed, 6600 + int(signed))
    rng = np.random.Generator(np.random.PCG64(66 + int(signed)))
    return np.ascontiguousarray(b[rng.permutation(len(b))])


def bc6h_cases(signed):
    kind = "bc6hs" if signed else "bc6hu"
    return [("%s_%s" % (kind, on), kind, bc6h_blocks(signed), _bytes(o), None) for on, o in bc6h_options().items()]


@functools.lru_cache(maxsize=None)
def etc_blocks(punchthrough):
    half = content.etc_half_blocks(8800)
    if punchthrough:
        return np.concatenate([half, content.punchthrough_blocks(8803, 1), content.dark_blocks(8802, 32)])
    return np.concatenate([half, content.mixed_ldr_blocks(8801, 16), content.dark_blocks(8802, 32)])


@functools.lru_cache(maxsize=None)
def eac_alpha_blocks():
    v = content.eac_directed_blocks(8810)
    b = np.full((len(v), 16, 4), 128, np.uint8)
    b[..., 3] = v
    return b


@functools.lru_cache(maxsize=None)
def r11_blocks(signed):
    return np.concatenate([content.eac_to_r11(content.eac_directed_blocks(8810), signed),
                           content.r11_narrow_blocks(8811, 256, signed)])


@functools.lru_cache(maxsize=None)
def s3tc_blocks():
    return np.concatenate([content.alpha_structure_blocks(8820, 256), content.mixed_ldr_blocks(8821, 16)])


ETC_KINDS = ("etc2", "etc2rgba", "etc1", "etc2punchthrough")
EAC_KINDS = ("eac", "r11u", "r11s")
S3TC_KINDS = ("bc1", "bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s")
_ETC_MODE = {"etc2": 0, "etc2rgba": 1, "eac": 2, "etc1": 3, "etc2punchthrough": 4}
_S3TC_CODE = {"bc2": 2, "bc3": 3, "bc4u": 4, "bc4s": 5, "bc5u": 6, "bc5s": 7}


def simple_case(kind):
    """the one case (default Options) of an ETC / EAC / S3TC format"""
    if kind in ETC_KINDS:
        blocks = etc_blocks(kind == "etc2punchthrough")
    elif kind == "eac":
        blocks = eac_alpha_blocks()
    elif kind in ("r11u", "r11s"):
        blocks = r11_blocks(kind == "r11s")
    else:
        blocks = s3tc_blocks()
    return (kind + "_default", kind, blocks, _bytes(api.Options()), None)


def etc_options():
    """the option sets that reach the FAKE instantiations of the ETC kernel (table and accurate rounding, with and without the
    uniform metric under it) and the two non-default weighted metrics"""
    F = api.Flags
    return {"fake": api.Options(flags=F.Default | F.ETC_UseFakeBT709),
            "fake_accurate": api.Options(flags=F.Ultra | F.ETC_UseFakeBT709),
            "fake_uniform": api.Options(flags=F.Default | F.ETC_UseFakeBT709 | F.Uniform),
            "uniform": api.Options(flags=F.Default | F.Uniform),
            "weights": api.Options(redWeight=0.1, greenWeight=1.0, blueWeight=0.8, alphaWeight=1.0)}


@functools.lru_cache(maxsize=None)
def etc_option_blocks(punchthrough):
    """etc_blocks plus the content that keeps the T mode's larger distances alive under the fake-BT.709 metric"""
    return np.concatenate([etc_blocks(punchthrough), content.fake709_t_blocks(8804)])


def etc_option_cases(kind=None):
    """every ETC colour format on its directed content under etc_options().  Not part of all_cases(): tests/golden/mode_census.npz
    holds the default Options only"""
    return [("%s_%s" % (k, on), k, etc_option_blocks(k == "etc2punchthrough"), _bytes(o), None)
            for k in ETC_KINDS if kind in (None, k) for on, o in etc_options().items()]


def all_cases():
    out = []
    for key in bc7_sets():
        out += bc7_cases(key)
    for signed in (False, True):
        out += bc6h_cases(signed)
    out += [simple_case(k) for k in ETC_KINDS + EAC_KINDS + S3TC_KINDS]
    return out


def source_for(kind, blocks):
    """the blocks as the encoder of `kind` reads them (the signed S3TC formats take the same bytes as int8)"""
    return blocks.view(np.int8) if kind in ("bc4s", "bc5s") else blocks


def encode_oracle(orc, case, rcp, threads=8):
    """the C restatement on one case"""
    _, kind, blocks, ob, pb = case
    if kind == "bc7":
        return orc.encode_bc7(blocks, ob, pb, rcp, threads)
    if kind in ("bc6hu", "bc6hs"):
        return orc.encode_bc6h(blocks, ob, kind == "bc6hs", rcp, threads)
    if kind in _ETC_MODE:
        return orc.encode_etc2(blocks, ob, _ETC_MODE[kind], threads)
    if kind in ("r11u", "r11s"):
        return orc.encode_eac11(blocks, kind == "r11s")
    if kind == "bc1":
        return orc.encode_bc1(blocks, ob, rcp, threads)
    return orc.encode_s3tc(blocks, ob, _S3TC_CODE[kind], rcp, threads)


def encode_reference(ref, case):
    """the reference itself (oracle/_ref) on one case"""
    _, kind, blocks, ob, pb = case
    if kind == "bc7":
        return ref.encode_bc7(blocks, ob, pb)
    if kind in ("bc6hu", "bc6hs"):
        return ref.encode_bc6h(blocks, ob, kind == "bc6hs")
    if kind in _ETC_MODE:
        return ref.encode_etc2(blocks, ob, _ETC_MODE[kind])
    if kind in ("r11u", "r11s"):
        return ref.encode_eac11(blocks, ob, kind == "r11s")
    if kind == "bc1":
        return ref.encode_bc1(blocks, ob)
    return ref.encode_s3tc(blocks, ob, _S3TC_CODE[kind])


def encode_gpu(ctx, case, blocks=None):
    """the kernels on one case; `blocks`: the case's blocks in another form (a device tensor, a prefix)"""
    _, kind, case_blocks, ob, pb = case
    blocks = case_blocks if blocks is None else blocks
    plan = api.BC7EncodingPlan.frombytes(pb) if pb is not None else None
    if isinstance(blocks, np.ndarray):
        blocks = source_for(kind, blocks)
    return ctx.encode(kind, blocks, api.Options.frombytes(ob), plan)
