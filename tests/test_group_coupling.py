"""Group coupling: the reference encodes eight blocks per call, and at a handful of AnySet / AllSet sites
one block's bytes depend on the other seven.  Every kernel restates that with hand-written cross-lane code.  These tests hold
it to inputs on which each site CHANGES bytes, at every placement of a group inside a wave at which that code can go wrong.

The inputs are tests/golden/group_coupling.npz, written by tools/find_coupling_witnesses.py: per site, witness groups W (a
witness is a block whose bytes change when the restatement's `site_mask` makes that one site see the block's own flag only),
neighbour groups N+ / N- with the site's predicate true / false in every block, the restatement's bytes (= the reference's)
and the per-block witness mask.

CPU: the fixture against its generator and against the reference (oracle/_ref, where built), its manifest against the
conditions a site needs to count as proven, group-wise streams, and the "benign" column of App. B checked instead of assumed.
GPU: every site's groups through the host path and a device tensor at the placements below; expected bytes come from the
fixture only, under the fixture's RCPPS table."""
import ctypes
import json
import os

import numpy as np
import pytest

import content
import fuzz_options
from oracle import pyref
from test_mode_census import _labels, _threads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIX = np.load(os.path.join(GOLD, "group_coupling.npz"))
MANIFEST = json.loads(str(FIX["manifest"]))
ENTRIES = list(MANIFEST["entries"])

MIN_GROUPS, MIN_POSITIONS, EMPTY_BUDGET = 8, 4, 16384
# sites shown reachable when the search was specified: each of these entries, and one entry of every tuple, has witnesses
MUST_HAVE = ("bc7_allow_rgb", "bc7_punch_commit", "etc2_opaque_tmax", "bc1_test_counts")
ONE_OF = (("bc6h_dup_skip_u", "bc6h_commit_loop_u"), ("bc6h_dup_skip_s", "bc6h_commit_loop_s"), ("etc2_punch_tmax", "etc2_punch_alpha"))


class Entry:
    """one entry of the fixture: its groups, bytes and the encoder they go through"""

    def __init__(self, name):
        m = MANIFEST["entries"][name]
        self.name, self.site, self.kind = name, m["site"], m["kind"]
        self.signed, self.mode = m["signed"], m["mode"]
        self.bit = pyref.SITES[self.site][0]
        self.src, self.role, self.wit = FIX["src_" + name], FIX["role_" + name], FIX["wit_" + name]
        self.opt = FIX["opt_" + name]
        self.plan = FIX["plan_" + name] if "plan_" + name in FIX.files else None
        self.fmt = {"bc7": "bc7", "bc1": "bc1", "bc6h": "bc6hs" if self.signed else "bc6hu",
                    "etc2": {0: "etc2", 4: "etc2punchthrough"}.get(self.mode)}[self.kind]

    def out(self, tag=None):
        return FIX["out_%s" % self.name if tag is None else "out_%s_%s" % (tag, self.name)]

    def variant_opt(self, tag):
        return self.opt if tag is None else FIX["opt_%s_%s" % (tag, self.name)]

    def variants(self):
        """tags of the further encodes of these groups the fixture holds (tools/find_coupling_witnesses.py variants())"""
        return [k[len("out_"):-len(self.name) - 1] for k in FIX.files if k.startswith("out_") and k.endswith("_" + self.name) and k != "out_" + self.name]

    def groups(self, *roles):
        return [int(g) for g in np.flatnonzero(np.isin(self.role, roles))]

    def take(self, array, seq):
        a = array.reshape((len(self.role), 8) + array.shape[1:])
        return np.ascontiguousarray(a[list(seq)].reshape((len(seq) * 8,) + array.shape[1:]))

    def encode(self, orc, blocks, site_mask=0, tag=None, threads=None):
        """the restatement on whole groups; tag: one of variants()"""
        t = threads or _threads()
        opt = self.variant_opt(tag)
        if self.kind == "bc7":
            return orc.encode_bc7(blocks, opt, self.plan, FIX["rcp"], t, site_mask=site_mask)
        if self.kind == "bc6h":
            return orc.encode_bc6h(blocks, opt, self.signed, FIX["rcp"], t, site_mask=site_mask)
        if self.kind == "bc1":
            return orc.encode_bc1(blocks, opt, FIX["rcp"], t, site_mask=site_mask)
        mode = 1 if tag in ("rgba", "rgba_alloc") else self.mode
        alloc = FIX["alloc_options"] if tag in ("alloc", "rgba_alloc") else None
        return orc.encode_etc2(blocks, opt, mode, t, alloc_options=alloc, site_mask=site_mask)

    def encode_ref(self, ref, blocks):
        if self.kind == "bc7":
            return ref.encode_bc7(blocks, self.opt, self.plan)
        if self.kind == "bc6h":
            return ref.encode_bc6h(blocks, self.opt, self.signed)
        if self.kind == "bc1":
            return ref.encode_bc1(blocks, self.opt)
        return ref.encode_etc2(blocks, self.opt, self.mode)


_ENTRY = {}


def entry(name):
    if name not in _ENTRY:
        _ENTRY[name] = Entry(name)
    return _ENTRY[name]


def witness_groups(e):
    """(number of witness groups, set of positions index & 7 that hold a witness) among the role-0 groups"""
    w = e.wit.reshape(-1, 8)[e.role == 0] > 0
    return int(w.any(axis=1).sum()), {int(p) for p in np.flatnonzero(w.any(axis=0))}


def proven(e):
    n, pos = witness_groups(e)
    return n >= MIN_GROUPS and len(pos) >= MIN_POSITIONS


# ------------------------------------------------------------------------------------------------ CPU: the fixture

def test_fixture_is_small_and_covers_every_site():
    assert os.path.getsize(os.path.join(GOLD, "group_coupling.npz")) < os.path.getsize(os.path.join(GOLD, "mode_census.npz"))
    assert {MANIFEST["entries"][n]["site"] for n in ENTRIES} == set(pyref.SITES)
    for n in ENTRIES:
        e = entry(n)
        assert len(e.src) == len(e.role) * 8 == len(e.wit) == len(e.out()), n   # whole groups only
        assert e.groups(1) and e.groups(2), n


@pytest.mark.parametrize("name", ENTRIES)
def test_manifest_conditions(name):
    """a site counts as proven with at least 8 witness groups whose witnesses sit at 4 or more positions of their group; only the
    sites that could not be checked when the search was specified may be empty, and then after 16 384 groups"""
    e, m = entry(name), MANIFEST["entries"][name]
    n, pos = witness_groups(e)
    assert m["kept"] == len(e.groups(0))
    if proven(e):
        return
    must = name in MUST_HAVE or any(name in grp and not any(proven(entry(o)) for o in grp if o != name) for grp in ONE_OF)
    assert not must, "%s: %d witness groups at positions %s" % (name, n, sorted(pos))
    assert m["may_be_empty"], "%s may not be left without witnesses (%d groups at positions %s)" % (name, n, sorted(pos))
    assert n == 0 and m["groups_searched"] >= EMPTY_BUDGET, (name, n, m["groups_searched"])


@pytest.mark.parametrize("name", ["bc7_any_alpha", "bc7_allow_rgb"])
def test_bc7_boolean_witnesses_are_attributable(name):
    """witnesses whose only coupled input is one mate: an opaque block in a group with a single block with alpha (its own
    allowRGBModes is the group's), or a block with minAlpha <= 250 in a group with a single block above 250 (its own
    anyBlockHasAlpha is the group's)"""
    e = entry(name)
    if not proven(e):   # only anyBlockHasAlpha may be empty, and test_manifest_conditions holds it to its search size
        assert name == "bc7_any_alpha" and witness_groups(e)[0] == 0
        return
    attr = FIX["attr_" + name].reshape(-1, 8) > 0
    mn = e.src[..., 3].min(axis=1).reshape(-1, 8)
    wit = e.wit.reshape(-1, 8) > 0
    assert attr.any(axis=1).sum() >= MIN_GROUPS and len(np.flatnonzero(attr.any(axis=0))) >= MIN_POSITIONS
    assert not (attr & ~wit).any()
    for g, p in zip(*np.nonzero(attr)):
        if name == "bc7_any_alpha":
            assert mn[g, p] == 255 and (mn[g] < 255).sum() == 1, (g, p, mn[g])
        else:
            assert mn[g, p] <= 250 and (mn[g] > 250).sum() == 1 and (mn[g] < 255).sum() == 7, (g, p, mn[g])


@pytest.mark.parametrize("name", ENTRIES)
def test_fixture_against_its_generator(oracle_lib, name):
    """mask 0 reproduces every expected block (every variant too); the site's mask changes exactly the marked blocks"""
    e = entry(name)
    assert (e.encode(oracle_lib, e.src) == e.out()).all()
    for tag in e.variants():
        assert (e.encode(oracle_lib, e.src, tag=tag) == e.out(tag)).all(), tag
    changed = (e.encode(oracle_lib, e.src, e.bit) != e.out()).any(axis=1)
    assert (changed == (e.wit > 0)).all(), np.flatnonzero(changed != (e.wit > 0))
    # a bit of another encoder family is no site of this one
    other = next(b for b, fam in pyref.SITES.values() if fam != e.kind)
    assert (e.encode(oracle_lib, e.src, other) == e.out()).all()


@pytest.mark.parametrize("name", ENTRIES)
def test_streams_are_group_wise(oracle_lib, name):
    """all the groups in one call = the concatenation of one call per group, in any order (the GPU streams rely on it)"""
    e = entry(name)
    per_group = np.concatenate([e.encode(oracle_lib, e.take(e.src, [g]), threads=1) for g in range(len(e.role))])
    assert (per_group == e.out()).all()
    seq = list(np.random.Generator(np.random.PCG64(3)).permutation(len(e.role)))
    assert (e.encode(oracle_lib, e.take(e.src, seq)) == e.take(e.out(), seq)).all()


@pytest.mark.parametrize("name", ENTRIES)
def test_reference_gives_the_expected_bytes(ref_lib, name):
    e = entry(name)
    assert (e.encode_ref(ref_lib, e.src) == e.out()).all()
    if "ref_" + name in FIX.files:   # the reference's bytes recorded when the fixture was made
        assert (FIX["ref_" + name] == e.out()).all()


# ------------------------------------------------------------------------------------------------ CPU: the benign column

BENIGN = ("bc1", "bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s", "etc1", "eac", "r11u", "r11s")
BENIGN_BLOCKS = 4096


def _benign_options():
    """default Options and three of the fuzz sets (a negative weight; nine refine rounds and six seed points; Ultra with
    punch-through, Uniform and a threshold above 1)"""
    sets = fuzz_options.options_sets(10)
    return [np.frombuffer(o.tobytes(), np.uint8).copy() for o in (fuzz_options.api.Options(), sets[2], sets[7], sets[9])]


def _benign_encode(lib, fmt, blocks, opt):
    is_ref = isinstance(lib, pyref.RefLib)
    kw = {} if is_ref else {"threads": _threads()}
    if fmt == "bc1":
        o = opt.copy()
        o[0:4] = np.frombuffer(np.uint32(int(o[0:4].view(np.uint32)[0]) & ~pyref.FLAG_S3TC_EXHAUSTIVE).tobytes(), np.uint8)
        return lib.encode_bc1(blocks, o, **kw)
    if fmt in ("bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s"):
        return lib.encode_s3tc(blocks, opt, 2 + ("bc2", "bc3", "bc4u", "bc4s", "bc5u", "bc5s").index(fmt), **kw)
    if fmt in ("etc1", "eac"):
        return lib.encode_etc2(blocks, opt, 3 if fmt == "etc1" else 2, **kw)
    return lib.encode_eac11(blocks, opt, fmt == "r11s") if is_ref else lib.encode_eac11(blocks, fmt == "r11s")


def _benign_check(lib, fmt):
    rng = np.random.Generator(np.random.PCG64(20261020))
    if fmt.startswith("r11"):
        blocks = content.mixed_r11_blocks(11, BENIGN_BLOCKS // 8)
    else:
        blocks = np.concatenate([content.mixed_ldr_blocks(808, BENIGN_BLOCKS // 16), content.alpha_structure_blocks(9, BENIGN_BLOCKS // 2)])
    assert len(blocks) == BENIGN_BLOCKS
    perm = rng.permutation(BENIGN_BLOCKS)
    assert (perm // 8 != np.arange(BENIGN_BLOCKS) // 8).mean() > 0.99   # nearly every block gets seven new mates
    for i, opt in enumerate(_benign_options()):
        a = _benign_encode(lib, fmt, blocks, opt)
        b = _benign_encode(lib, fmt, np.ascontiguousarray(blocks[perm]), opt)
        bad = np.flatnonzero((a[perm] != b).any(axis=1))
        assert bad.size == 0, "%s, options set %d: %d blocks depend on their group, first %s" % (fmt, i, bad.size, perm[bad[:8]])
        if fmt.startswith("r11"):
            break   # EncodeETC2Alpha11 reads no Options


@pytest.mark.parametrize("fmt", BENIGN)
def test_benign_formats_do_not_depend_on_the_group(oracle_lib, fmt):
    """BC1 without S3TC_Exhaustive, BC2 to BC5, ETC1, ETC2 alpha and R11: the kernels treat them as lane-independent.  The same
    blocks dealt to other groups must get the same bytes"""
    _benign_check(oracle_lib, fmt)


@pytest.mark.parametrize("fmt", BENIGN)
def test_benign_formats_do_not_depend_on_the_group_in_the_reference(ref_lib, fmt):
    _benign_check(ref_lib, fmt)


# ------------------------------------------------------------------------------------------------ GPU

PLACEMENTS = ("alone", "W,N", "N,W", "N,N,W", "interleaved72", "interleaved264")


def interleaved(e, groups):
    """W N+ W N- W N+ ...: `groups` groups, cycling through the entry's witness and neighbour groups"""
    W, NP, NM = e.groups(0), e.groups(1), e.groups(2, 3)
    seq, w, p, m = [], 0, 0, 0
    while len(seq) < groups:
        seq.append(W[w % len(W)])
        w += 1
        if len(seq) < groups:
            if w & 1:
                seq.append(NP[p % len(NP)])
                p += 1
            else:
                seq.append(NM[m % len(NM)])
                m += 1
    return seq


def streams(e, placement):
    """the group sequences of one placement: lists of group indices into the entry's arrays"""
    W, NP, NM = e.groups(0), e.groups(1), e.groups(2, 3)
    if placement == "alone":           # one call of 8 blocks
        return [[w] for w in W]
    if placement in ("W,N", "N,W"):    # both 32-lane halves of a BC7 / BC6H wave, beside a neighbour that would corrupt a 64-lane ballot
        pairs = [(w, n) for i, w in enumerate(W) for n in (NP[i % len(NP)], NM[i % len(NM)])]
        return [[w, n] if placement == "W,N" else [n, w] for w, n in pairs]
    if placement == "N,N,W":           # 24 blocks: W in a half-empty last wave
        return [[NP[i % len(NP)], NM[i % len(NM)], w] for i, w in enumerate(W)]
    return [interleaved(e, int(placement[len("interleaved"):]) // 8)]


def check_stream(e, seq, got, exp, what):
    """every block equal; a failure names site, placement, path, the block's index, its group's role and its position"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero((got != exp).any(axis=1))
    if bad.size:
        first = bad[:6]
        kind = "etc2rgba" if exp.shape[1] == 16 and e.kind == "etc2" else e.fmt
        want, have = _labels(kind, exp[first]), _labels(kind, got[first])
        role = ("W", "N+", "N-", "N- (derived)")
        lines = ["block %d (group %d of the stream = fixture group %d, %s; position %d in its group%s): expected %s, got %s"
                 % (i, i // 8, seq[i // 8], role[e.role[seq[i // 8]]], i & 7, ", a witness" if e.wit[seq[i // 8] * 8 + (i & 7)] else "", w, h)
                 for i, w, h in zip(first, want, have)]
        pytest.fail("site %s (%s), %s: %d of %d blocks differ\n  %s" % (e.site, e.name, what, bad.size, len(exp), "\n  ".join(lines)))


def _api():
    from convectionkernels_amd import api
    return api


def gpu_variants(e):
    """(label, format, fixture tag, exhaustive, allocated-with Options or None) of every encode the entry's groups go through"""
    api = _api()
    if e.kind == "bc7":
        return [("pruned", "bc7", None, False, None), ("exhaustive", "bc7", None, True, None)]
    if e.kind == "bc6h":
        return [("default", e.fmt, None, False, None), ("fast indexing, 3 seed points", e.fmt, "fast", False, None)]
    if e.kind == "bc1":
        return [("Flags::Better", "bc1", None, False, None)]
    alloc = api.Options.frombytes(FIX["alloc_options"])
    v = [(e.fmt, e.fmt, None, False, None), ("with_data " + e.fmt, e.fmt, "alloc", False, alloc)]
    if e.mode == 0:
        v += [("etc2rgba", "etc2rgba", "rgba", False, None), ("with_data etc2rgba", "etc2rgba", "rgba_alloc", False, alloc)]
    return v


def run_paths(ctx, e, fmt, blocks, opt, plan, alloc):
    """path name -> packed bytes: the host path, a device tensor, and for the with_data kinds the named device entry point of
    tests/test_buffer_contract.py"""
    import torch
    out = {"host": ctx.encode(fmt, blocks, opt, plan, compression_data=alloc)}
    t = torch.from_numpy(blocks).cuda()
    out["device"] = ctx.encode(fmt, t, opt, plan, compression_data=alloc).cpu().numpy()
    if alloc is not None:
        import test_buffer_contract as B
        assert B._opt_bytes(B._ALLOC_OPT).tobytes() == FIX["alloc_options"].tobytes()
        name = {"etc2": "with_data_rgb", "etc2rgba": "with_data_rgba", "etc2punchthrough": "with_data_punchthrough"}[fmt]
        _, _, out_bpb, call, _, _ = B.ENCODERS[name]
        res = torch.empty((len(blocks), out_bpb), dtype=torch.uint8, device=t.device)
        torch.cuda.synchronize()
        assert call(ctx._lib, ctx._h, res.data_ptr(), t.data_ptr(), len(blocks), opt) == 0
        torch.cuda.synchronize()
        out["device, " + name] = res.cpu().numpy()
    return out


@pytest.fixture()
def ctx(gpu_ctx):
    """the shared context under the fixture's RCPPS table (put back afterwards)"""
    saved = gpu_ctx.get_rcp_table()
    gpu_ctx.set_rcp_table(FIX["rcp"])
    yield gpu_ctx
    gpu_ctx.set_exhaustive(False)
    gpu_ctx.set_rcp_table(saved)


def run_placement(ctx, e, placement, only_variants=None):
    api = _api()
    plan = api.BC7EncodingPlan.frombytes(e.plan) if e.plan is not None else None
    for label, fmt, tag, exhaustive, alloc in gpu_variants(e):
        if only_variants is not None and label not in only_variants:
            continue
        opt = api.Options.frombytes(e.variant_opt(tag))
        ctx.set_exhaustive(exhaustive)
        for seq in streams(e, placement):
            blocks, exp = e.take(e.src, seq), e.take(e.out(tag), seq)
            for path, got in run_paths(ctx, e, fmt, blocks, opt, plan, alloc).items():
                check_stream(e, seq, got, exp, "placement %s %s, %s, path %s" % (placement, seq if len(seq) < 4 else "(%d blocks)" % len(blocks), label, path))
        ctx.set_exhaustive(False)


@pytest.mark.gpu
@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("name", ENTRIES)
def test_gpu_site_at_every_placement(ctx, name, placement):
    """W alone (8 blocks); [W, N] and [N, W] for N in {N+, N-} (16 blocks: either half of a wave); [N, N, W] (24 blocks: a
    half-empty last wave); W interleaved with alternating N+ / N- at 72 and 264 blocks"""
    run_placement(ctx, entry(name), placement)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in ENTRIES if MANIFEST["entries"][n]["kind"] == "etc2"])
def test_gpu_etc2_129_groups(ctx, name):
    """1032 blocks: 129 groups are no multiple of the eight XCDs the ETC2 block map deals groups to"""
    run_placement(ctx, entry(name), "interleaved1032")


def _hard_stats(ctx):
    lib = ctx._lib
    lib.cvttmi_bc7_hard_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    n, slots = ctypes.c_uint32(), ctypes.c_uint32()
    assert lib.cvttmi_bc7_hard_stats(ctx._h, ctypes.byref(n), ctypes.byref(slots)) == 0
    return n.value, slots.value


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bc7_any_alpha", "bc7_allow_rgb"])
def test_gpu_bc7_second_launch_keeps_the_group_flags(name, monkeypatch):
    """a context with a hand-over slot for every block (as test_bc7_gpu.test_second_launch_hand_over_is_invisible makes it): a
    block finished by the second launch must still be encoded under its group's two booleans.  The counters say how many
    blocks were handed over, not which; the number is printed and the assertion is on the bytes"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    api = _api()
    for k in ("CVTTMI_BC7_HARD_MIN", "CVTTMI_BC7_HARD_CAP", "CVTTMI_BC7_HARD_DIV"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CVTTMI_BC7_HARD_CAP", "4096")
    monkeypatch.setenv("CVTTMI_BC7_HARD_MIN", "2")
    hard = api.Context(0)   # the settings are read when the context is created
    hard.set_rcp_table(FIX["rcp"])
    e = entry(name)
    opt, plan = api.Options.frombytes(e.opt), api.BC7EncodingPlan.frombytes(e.plan)
    for placement in ("W,N", "interleaved264"):
        for seq in streams(e, placement):
            blocks, exp = e.take(e.src, seq), e.take(e.out(), seq)
            got = hard.encode_bc7(torch.from_numpy(blocks).cuda(), opt, plan).cpu().numpy()
            handed, slots = _hard_stats(hard)
            if len(seq) > 2:
                print("%s, %d blocks: %d handed to the second launch (%d slots)" % (name, len(blocks), handed, slots))
            check_stream(e, seq, got, exp, "placement %s, hand-over context, path device" % placement)
            check_stream(e, seq, hard.encode_bc7(blocks, opt, plan), exp, "placement %s, hand-over context, path host" % placement)


@pytest.mark.gpu
def test_gpu_bc7_punch_commit_in_several_launches(monkeypatch):
    """seven refine rounds keep the punch-through trial table in HBM, and the table cap of
    test_bc7_gpu.test_respect_punchthrough_chunked_launches (10 waves a launch) cuts 264 blocks into 160 + 104: the commit rule's
    8-lane slices must still line up with the groups in the second, ragged launch"""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    api = _api()
    monkeypatch.setenv("CVTTMI_BC7_PT_TABLE_KB", "140")
    small = api.Context(0)
    monkeypatch.delenv("CVTTMI_BC7_PT_TABLE_KB")
    small.set_rcp_table(FIX["rcp"])
    e = entry("bc7_punch_commit")
    opt, plan = api.Options.frombytes(e.variant_opt("refine7")), api.BC7EncodingPlan.frombytes(e.plan)
    assert opt.refineRoundsBC7 == 7
    for exhaustive in (False, True):
        small.set_exhaustive(exhaustive)
        for placement in ("W,N", "N,W", "interleaved264"):
            for seq in streams(e, placement):
                blocks, exp = e.take(e.src, seq), e.take(e.out("refine7"), seq)
                what = "placement %s, 7 refine rounds, table cap 140 KB, %s" % (placement, "exhaustive" if exhaustive else "pruned")
                check_stream(e, seq, small.encode_bc7(blocks, opt, plan), exp, what + ", path host")
                check_stream(e, seq, small.encode_bc7(torch.from_numpy(blocks).cuda(), opt, plan).cpu().numpy(), exp, what + ", path device")
