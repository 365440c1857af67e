"""CPU tests: the C restatement (oracle/cvtt_oracle.c) against the committed golden vectors
(generated with the real reference by tests/golden/make_golden.py) and, where oracle/_ref was
built, against the reference itself on fresh inputs."""
import os

import numpy as np
import pytest

import content
from oracle import pyref

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _mode_of(block):
    b0 = int(block[0])
    return (b0 & -b0).bit_length() - 1


def test_known_answers_bc7(oracle_lib):
    g = np.load(os.path.join(GOLD, "known_answers.npz"))
    out = oracle_lib.encode_bc7(g["blocks"], pyref.make_options(), _default_plan_bytes(), g["rcp"])
    assert (out == g["bc7"]).all()
    # SURVEY.md App. H, first and last block
    assert out[0].tobytes().hex() == "108a856ce10f2c7dcac90b5c0a5d2acf"
    assert out[7].tobytes().hex() == "503cfc0f29c283570bd68ac6fad0faac"


def _default_plan_bytes():
    from convectionkernels_amd import api
    return np.frombuffer(api.BC7EncodingPlan().tobytes(), np.uint8).copy()


def test_default_pods_match_golden():
    from convectionkernels_amd import api
    g = np.load(os.path.join(GOLD, "bc7_mixed.npz"))
    assert api.Options().tobytes() == g["opt_default"].tobytes()
    assert api.BC7EncodingPlan().tobytes() == g["plan_default"].tobytes()


@pytest.mark.parametrize("name", ["default", "uniform", "punchthrough", "better", "ultra", "singlecolor", "refine1", "refine3", "weights",
                                  "quality1", "quality20", "quality60", "quality100"])
def test_golden_mixed(oracle_lib, name):
    g = np.load(os.path.join(GOLD, "bc7_mixed.npz"))
    out = oracle_lib.encode_bc7(g["blocks"], g["opt_" + name], g["plan_" + name], g["rcp"], threads=8)
    bad = np.nonzero((out != g["out_" + name]).any(axis=1))[0]
    assert bad.size == 0, "blocks %s differ" % bad[:8]


def test_golden_covers_all_modes():
    g = np.load(os.path.join(GOLD, "bc7_mixed.npz"))
    modes = set()
    for n in ("default", "uniform"):
        modes |= {_mode_of(b) for b in g["out_" + n]}
    assert modes == set(range(8))


def test_config2_head(oracle_lib):
    """first 64 groups of BASELINE config 2 (4096^2 random RGBA, seed 2) and its opaque variant"""
    import json
    h = json.load(open(os.path.join(GOLD, "config_hashes.json")))
    rcp = np.array(h["rcp_hex"], np.uint32).view(np.float32)
    for key, opaque in (("config2_bc7_4096_seed2", False), ("config2b_bc7_4096_seed2_opaque", True)):
        head = np.load(os.path.join(GOLD, key + "_head.npy"))
        blocks = content.config_blocks(2, 4096, 4096, opaque=opaque)[:128]
        out = oracle_lib.encode_bc7(blocks, pyref.make_options(), _default_plan_bytes(), rcp, threads=8)
        assert (out == head[:128]).all()


def test_rcp_table_matters(oracle_lib):
    """exact 1/n instead of RCPPS changes outputs -- the table is a real input"""
    g = np.load(os.path.join(GOLD, "bc7_mixed.npz"))
    exact = np.array([1.0] + [1.0 / i for i in range(1, 17)], np.float32)
    out = oracle_lib.encode_bc7(g["blocks"], g["opt_default"], g["plan_default"], exact, threads=8)
    assert (out != g["out_default"]).any()


def test_group_coupling_is_modelled(oracle_lib):
    """a block's output may depend on its group (two alpha booleans): an opaque block next to
    alpha blocks is encoded with the RGBA seeds / mode-7 rules of BC67.cpp:1069-1078"""
    rng = np.random.Generator(np.random.PCG64(5))
    blocks = rng.integers(0, 256, (64, 16, 4)).astype(np.uint8)
    blocks[::2, :, 3] = 255
    opt, plan = pyref.make_options(), _default_plan_bytes()
    grouped = oracle_lib.encode_bc7(blocks, opt, plan)
    alone = np.zeros_like(grouped)
    for i in range(64):
        rep = np.repeat(blocks[i:i + 1], 8, axis=0)
        alone[i] = oracle_lib.encode_bc7(rep, opt, plan)[0]
    assert grouped.shape == alone.shape
    # on random content the coupling rarely flips a bit; on the witnesses of tests/golden/group_coupling.npz (blocks whose
    # bytes change when allowRGBModes / anyBlockHasAlpha see the block's own alpha only) it must
    g = np.load(os.path.join(GOLD, "group_coupling.npz"))
    for name in ("bc7_allow_rgb", "bc7_any_alpha"):
        src, wit = g["src_" + name], np.flatnonzero(g["wit_" + name])
        assert wit.size >= 8, name
        grouped = oracle_lib.encode_bc7(src, g["opt_" + name], g["plan_" + name], g["rcp"], threads=8)
        assert (grouped == g["out_" + name]).all(), name
        alone = oracle_lib.encode_bc7(np.repeat(src[wit], 8, axis=0), g["opt_" + name], g["plan_" + name], g["rcp"], threads=8)[::8]
        same = wit[(alone == grouped[wit]).all(axis=1)]
        assert same.size == 0, "%s: witnesses %s encode alone as they do in their group" % (name, same)


def test_against_reference_fresh_inputs(oracle_lib, ref_lib):
    blocks = content.mixed_ldr_blocks(99, 12)
    rcp = ref_lib.probe_rcp()
    for opt in (pyref.make_options(), pyref.make_options(flags=pyref.FLAGS_BETTER | pyref.FLAG_UNIFORM)):
        a = ref_lib.encode_bc7(blocks, opt, ref_lib.default_plan())
        b = oracle_lib.encode_bc7(blocks, opt, ref_lib.default_plan(), rcp, threads=8)
        assert (a == b).all()


def test_single_colour_tables_are_generated_from_the_rule():
    """oracle/cvtt_oracle_bc7sc.h is what tools/gen_bc7_single_color.py emits (spot checks of the rule)"""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    spec = importlib.util.spec_from_file_location("gen_sc", os.path.join(root, "tools", "gen_bc7_single_color.py"))
    sc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sc)
    idx, pbits, ent = sc.table(7, 1, 0, 0, 1, 15)  # mode 6, p-bits 0, index 1
    assert (idx, pbits) == (1, 0) and ent[0] == (0, 0, 0) and len(ent) == 256
    for v in (0, 17, 128, 255):
        lo, hi, c = ent[v]
        assert c == ((64 - 4) * lo + 4 * hi + 32) >> 6 and abs(c - v) <= 1
    text = open(os.path.join(root, "oracle", "cvtt_oracle_bc7sc.h")).read()
    assert "ORC_BC7SC_NUM_TABLES 39" in text
