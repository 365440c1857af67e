"""Every value the BC7 kernel compares with a block's best error in order to drop a candidate, read from the kernel itself and
held to two independent references (tests/bc7_bound_ref.py):

  A  the exact bound in float64 -- what "Soundness of the bounds" (docs/history.md) derives: computed <= sum over the subsets
     of g(R) + the static alpha error, stored <= computed, no tolerance; the sharp bounds against `sharp_bound` with the
     direction the kernel used.  Only for option sets whose four weights are positive.
  B  soundness itself: the value <= E * (1 + 20 * 2^-24), E = the error the reference reaches for the candidate the value
     stands for (a plan that leaves that one candidate, the C restatement's bytes decoded and measured in float64), at every
     site that forms, stores, reads back or compares a bound, for the mode it was compared for.

The values come from the bound-dump build of the library (bc7_kernel.hip, CVTT_BC7_BOUND_DUMP; a variant `make` builds next to
the default library), loaded in one child process; its output must be the oracle's bytes, so it is the kernel that ships with
one record per bound added.  The second launch (HARD) runs without bounds -- the first launch has applied them -- so its only
records are final errors.  The CPU tests pin what the references rest on: the C restatement to the real reference on the
single-candidate plans (tests/golden/bc7_single_candidate.npz), the decoder, the exact bound on hand-computed subsets, the
truncation of the bound table, and that every candidate is emitted as asked on the content of the GPU tests."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bc7_bound_ref as R
from convectionkernels_amd import api, synth
from test_bc7_bound_trim_gpu import FAMILY_OPTIONS, subset_edge_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DUMP_LIB = os.path.join(ROOT, "convectionkernels_amd", "lib", "variants", "libcvtt_mi355x_bounddump.so")
REPORT = os.path.join(ROOT, "profiles", "bounds", "bound_soundness.json")
TOL_B = 1.0 + 20.0 * R.U24  # the 20 u "Soundness of the bounds" gives for the reference's own error sums
HAND_OVER = {"CVTTMI_BC7_HARD_CAP": "4096", "CVTTMI_BC7_HARD_MIN": "2"}  # as test_second_launch_hand_over_is_invisible forces it

# name -> (Options, environment of the context, does reference A apply)
OPTION_SETS = {
    "default": (api.Options(), {}, True),
    "uniform": (api.Options(flags=api.Flags.Default | api.Flags.Uniform), {}, True),
    "spread": (api.Options(redWeight=100.0, greenWeight=1e-3, blueWeight=0.1, alphaWeight=3.0), {}, True),
    "weights": (api.Options(**FAMILY_OPTIONS["weights"]), {}, False),  # (-1, 0, 100, 1): reference B only
    "better": (api.Options(flags=api.Flags.Better), {}, True),
    "ultra_pt": (api.Options(flags=api.Flags.Ultra | api.Flags.BC7_RespectPunchThrough), {}, True),
    "hand_over": (api.Options(), HAND_OVER, True),
}
SIZES = (16, 24, 384)  # one wave; a second wave half valid; the whole set


@functools.lru_cache(maxsize=None)
def content_blocks():
    """8 families x 16 blocks (a wave each), then the 256 collinear / single-colour subset blocks: 384 blocks"""
    fam = synth.content_families(16, seed=11)
    blocks = np.concatenate([fam[k] for k in sorted(fam)] + [subset_edge_blocks(7)])
    assert blocks.shape == (384, 16, 4)
    return blocks


def _oracle():
    from oracle import pyref
    return pyref.OracleLib()


# ------------------------------------------------------------------------------------------------ CPU tests
def test_exact_bound_of_collinear_and_single_colour_subsets_is_zero():
    w = R.W_DEFAULT
    delta = 0.5 * np.sqrt((w ** 2).sum())
    single = np.tile(np.array([[17.0, 200.0, 3.0]]), (7, 1)) * w
    assert R.exact_subset_bound(single, delta) == 0.0
    line = (np.array([[10.0, 20.0, 30.0]]) + np.arange(9)[:, None] * np.array([[3.0, -2.0, 5.0]])) * w
    assert R.exact_subset_bound(line, delta) == 0.0
    # ... and a subset with a known residual: four corners of a square of side 2a in two channels of weight one.  The scatter
    # matrix is 4 a^2 I, R = 4 a^2, n = 4, delta = 0.5 sqrt(2): g = 4 a^2 - 2 delta sqrt(16 a^2) = 4 a^2 - 8 a delta
    a = 10.0
    sq = np.array([[a, a], [a, -a], [-a, a], [-a, -a]])
    d2 = 0.5 * np.sqrt(2.0)
    assert abs(R.exact_subset_bound(sq, d2) - (4 * a * a - 8 * a * d2)) < 1e-9
    # below the threshold R >= n delta^2 the bound is void
    tiny = np.array([[0.1, 0.1], [0.1, -0.1], [-0.1, 0.1], [-0.1, -0.1]])
    assert R.exact_subset_bound(tiny, d2) == 0.0
    # the table form agrees with the one-subset form, partition by partition
    blocks = content_blocks()[48:52]
    ex = R.ExactBounds(blocks, api.Options())
    tab = ex.subsets((0, 1, 2), 2)
    for b in range(len(blocks)):
        for part in (0, 13, 63):
            for s, m in enumerate(R.subset_masks(2, part)):
                pts = blocks[b][[p for p in range(16) if (m >> p) & 1]][:, :3].astype(np.float64) * ex.w[:3]
                assert abs(tab[b, part, s] - R.exact_subset_bound(pts, ex.delta((0, 1, 2)))) <= 1e-9 * max(1.0, tab[b, part, s])


def test_decoder_restatement_equals_the_reference_decoder():
    d = np.load(os.path.join(GOLD, "decode.npz"))
    assert (R.decode_bc7(d["bc7_in"]) == d["bc7_out"]).all()


def test_bound_table_truncation_never_rounds_up():
    """lbStore keeps the upper 16 bits of the binary32 value and readers take the absolute value: for every v >= 0 the table
    gives back a value <= v, within 2^-7 of it, and with the tier mark (the sign bit) the same value"""
    rng = np.random.Generator(np.random.PCG64(5))
    bits = np.concatenate([rng.integers(0, 0x7F800000, 200000, dtype=np.uint32),
                           np.array([0, 1, 0x0000FFFF, 0x00010000, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3F80FFFF, 0x7F7FFFFF], np.uint32)])
    v = bits.view(np.float32)
    back = R.lb_store(v)
    assert (back <= v).all()
    normal = v >= np.float32(2.0 ** -126)  # seven mantissa bits stay
    assert (back[normal].astype(np.float64) >= v[normal].astype(np.float64) * (1.0 - 2.0 ** -7)).all()
    assert (back.view(np.uint32) == (bits & np.uint32(0xFFFF0000))).all()
    marked = ((bits >> np.uint32(16)) | np.uint32(0x8000)).astype(np.uint32) << np.uint32(16)  # lbStoreTier2
    assert (np.abs(marked.view(np.float32)) == back).all()
    # the source says what this restates
    src = open(os.path.join(ROOT, "convectionkernels_amd", "csrc", "bc7_kernel.hip")).read()
    assert "s_bound[partition][b] = (unsigned short)(__builtin_bit_cast(u32, v) >> 16);" in src
    assert "return __builtin_fabsf(lbLoadRaw(partition, b));" in src


def test_oracle_equals_reference_on_single_candidate_plans():
    """the C restatement on the plans reference B uses, against bytes the real reference emitted (make_golden.py)"""
    g = np.load(os.path.join(GOLD, "bc7_single_candidate.npz"))
    orc = _oracle()
    cands = [(int(m), int(w)) for m, w in g["candidates"]]
    assert cands == R.candidates()
    ob = R._bytes(api.Options())
    in_class = _classes(g["blocks"])
    assert 16 <= in_class(0).sum() <= 48
    for i, (mode, which) in enumerate(cands):
        got = orc.encode_bc7(g["blocks"], ob, R._bytes(R.single_candidate_plan(mode, which)), g["rcp"], threads=4)
        # (a block whose group does not allow modes 0-3 commits nothing under such a plan: its bytes are not defined)
        cls = in_class(mode)
        assert R.emitted_as_asked(g["packed"][i], mode, which)[cls].all()
        assert (got[cls] == g["packed"][i][cls]).all(), "mode %d candidate %d: the C restatement differs from the reference" % (mode, which)


def _classes(blocks):
    allowed = R.rgb_modes_allowed(blocks)
    return lambda mode: allowed if mode < 4 else np.ones(len(blocks), bool)


@functools.lru_cache(maxsize=None)
def reached(name):
    """reference B of an option set on the whole content, and that every pair of the comparison is emitted as asked"""
    blocks = content_blocks()
    orc = _oracle()
    E = R.reached_errors(orc, blocks, OPTION_SETS[name][0], orc.probe_rcp(), threads=16)
    in_class = _classes(blocks)
    skipped = [(m, w, int(b)) for (m, w), (_, ok, _) in E.items() for b in np.nonzero(in_class(m) & ~ok)[0]]
    assert not skipped, "%s: %d pairs not emitted as asked, first (mode, candidate, block): %s" % (name, len(skipped), skipped[:8])
    return E


@pytest.mark.parametrize("name", [n for n in OPTION_SETS if n != "hand_over"])  # (hand_over: the Options of default)
def test_every_candidate_is_emitted_as_asked(name):
    """The content classes of reference B: every block for modes 4-7 (mode 7 is steered by seed counts, see
    single_candidate_plan), blocks whose group allows the RGB modes for modes 0-3.  0 skipped pairs; both kinds of block are
    in both classes."""
    blocks = content_blocks()
    E = reached(name)
    assert len(E) == 285
    allowed = R.rgb_modes_allowed(blocks)
    opaque = blocks[:, :, 3].min(1) == 255
    assert (allowed & opaque).sum() >= 100 and (allowed & ~opaque).sum() >= 20 and (~opaque).sum() >= 100
    for (m, w), (e, ok, _) in E.items():
        assert np.isfinite(e).all() and (e >= 0).all()


# ------------------------------------------------------------------------------------------------ GPU tests
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """one child process with the dump build: every option set x every size"""
    return run_dump_child(str(tmp_path_factory.mktemp("bound_dump")))


def run_dump_child(tmp, lib=None):
    """Starts tests/bc7_bound_dump_child.py on every option set x every size with the dump build `lib` loaded, under a time
    limit of its own, and returns what it wrote; the exit status is checked before anything is read.  `lib`: a developer's
    other dump build, by its path or through CVTT_BOUND_DUMP_LIB."""
    lib = lib or os.environ.get("CVTT_BOUND_DUMP_LIB", DUMP_LIB)
    assert os.path.exists(lib), "%s is missing: `make -C convectionkernels_amd/csrc` builds it" % lib
    np.save(os.path.join(tmp, "blocks.npy"), content_blocks())
    jobs = [{"name": "%s_%d" % (name, n), "n": n, "options": list(opt.tobytes()), "env": env}
            for name, (opt, env, _) in OPTION_SETS.items() for n in SIZES]
    spec = {"blocks": os.path.join(tmp, "blocks.npy"), "rcp": [int(x) for x in _oracle().probe_rcp().view(np.uint32)],
            "capacity": 1 << 20, "jobs": jobs}
    with open(os.path.join(tmp, "jobs.json"), "w") as f:
        json.dump(spec, f)
    env = dict(os.environ)
    env["CVTTMI_LIB"] = lib
    for k in HAND_OVER:
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "bc7_bound_dump_child.py"), os.path.join(tmp, "jobs.json"),
                        os.path.join(tmp, "out.npz")], env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, "the dump child ended with status %d\n%s\n%s" % (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    return np.load(os.path.join(tmp, "out.npz"))


_SHARP_CACHE = {}


def _sharp_ref(key, blocks, ex, rec):
    """reference A of one subset's sharp bound, with the direction the kernel recorded"""
    if key not in _SHARP_CACHE:
        ch = [0, 1, 2, 3] if rec["set"] == 0 else [0, 1, 2]
        m = R.subset_masks(int(rec["subsets"]), int(rec["part"]))[int(rec["sub"])]
        pts = blocks[int(rec["block"])][[p for p in range(16) if (m >> p) & 1]][:, ch].astype(np.float64) * ex.w[ch]
        d = rec["x"][:len(ch)].astype(np.float64)
        plain = float(ex.subsets(tuple(ch), int(rec["subsets"]))[int(rec["block"]), int(rec["part"]), int(rec["sub"])])
        if not d.any() or len(pts) < 3:
            _SHARP_CACHE[key] = plain
        else:
            _SHARP_CACHE[key] = max(plain, R.sharp_bound(pts, d / np.linalg.norm(d), 4 if rec["bits"] == 2 else 8, ex.w[ch]))
    return _SHARP_CACHE[key]


def _modes_held(rec):
    """(mode, candidate) pairs a record's value is held to (reference B)"""
    tier, kind, bset, bits, part = int(rec["tier"]), int(rec["kind"]), int(rec["set"]), int(rec["bits"]), int(rec["part"])
    if tier == R.T_ROT:
        if kind == R.K_RELOAD:  # compared for one configuration
            return [(4, 2 * part + bits)] if rec["mode"] == 4 else [(5, part)]
        return [(4, 2 * part), (4, 2 * part + 1), (5, part)]
    if kind == R.K_RELOAD or tier in (R.T_PROBE_FULL, R.T_PROBE_SHARP):
        modes = (int(rec["mode"]),)  # the mode whose stage read or formed it
    else:
        modes = R.SET_MODES[bset][bits]
    return [(m, 0 if m == 6 else part) for m in modes if not (m == 0 and part >= 16)]


def analyse(name, n, dump):
    """every assertion on one run; returns per-tier statistics"""
    opt, _, apply_a = OPTION_SETS[name]
    blocks = content_blocks()
    job = "%s_%d" % (name, n)
    count = int(dump["count_" + job][0])
    raw = np.ascontiguousarray(dump["records_" + job])
    assert count == len(raw), "%s: the dump overflowed (%d records, %d kept)" % (job, count, len(raw))
    rec = raw.view(R.RECORD_DTYPE).reshape(-1)
    assert (rec["block"] < n).all()
    # the dump build is the kernel that ships: its bytes are the oracle's
    orc = _oracle()
    exp = orc.encode_bc7(blocks[:n], R._bytes(opt), R._bytes(api.BC7EncodingPlan()), orc.probe_rcp(), threads=16)
    bad = np.nonzero((dump["packed_" + job] != exp).any(axis=1))[0]
    assert bad.size == 0, "%s: the dump build's output differs from the oracle at blocks %s" % (job, bad[:8])

    E = reached("default" if name == "hand_over" else name)
    in_class = _classes(blocks)
    ex = R.ExactBounds(blocks, opt)
    fin = rec[rec["kind"] == R.K_END]
    final = np.full(n, np.inf)
    np.minimum.at(final, fin["block"], fin["computed"].astype(np.float64))
    assert np.isfinite(final).all(), "%s: blocks without a final record" % job

    viol = []
    stats = {t: {"records": 0, "nonzero": 0, "dropped": 0, "max_stored_over_A": 0.0, "min_headroom_B": None, "pairs_B": 0,
                 "pairs_out_of_class": 0} for t in R.TIERS}
    body = rec[rec["kind"] <= R.K_RELOAD]
    for t, tname in enumerate(R.TIERS):
        sel = body[body["tier"] == t]
        stats[tname]["records"] = int(len(sel))
        stats[tname]["nonzero"] = int((sel["stored"] > 0).sum())
        stats[tname]["dropped"] = int((sel["dropped"] != 0).sum())
    # a dropped candidate is one whose value exceeds the best error, and the best error only falls
    cmpd = body[body["kind"] != R.K_FORM]
    compared = np.where(cmpd["kind"] == R.K_RELOAD, cmpd["stored"], cmpd["computed"])  # a fresh value is compared before it is truncated
    assert ((cmpd["dropped"] != 0) == (compared > cmpd["err"])).all(), "%s: a drop flag that is not `value > best error`" % job
    low = cmpd[cmpd["err"].astype(np.float64) < final[cmpd["block"]]]
    if len(low):
        viol.append("best error below the final error: %s" % low[:3])

    # ---- reference A
    if apply_a:
        prior = {}
        for bset in (0, 1, 2, 3):
            a_tab = ex.set_bound(bset)
            for tier in (R.T_WHOLE6, R.T_TIER1, R.T_FULL):
                s = body[(body["set"] == bset) & (body["tier"] == tier) & (body["kind"] <= R.K_FORM_CMP)]
                if not len(s):
                    continue
                a = a_tab[s["block"], np.minimum(s["part"], a_tab.shape[1] - 1)]
                over = s[s["computed"].astype(np.float64) > a]
                if len(over):
                    viol.append("A: computed above the exact bound, tier %s set %d: %s (exact %s)" % (R.TIERS[tier], bset, over[:3], a[s["computed"] > a][:3]))
                if tier == R.T_FULL:  # the table keeps the larger of the new value and the one it held
                    up = s[s["stored"] > np.maximum(s["computed"], prior[bset][s["block"], s["part"]])]
                else:
                    up = s[s["stored"] > s["computed"]]
                if tier != R.T_WHOLE6:
                    tab = prior.setdefault(bset, np.zeros((n, 64), np.float32))
                    np.maximum.at(tab, (s["block"], s["part"]), s["computed"])
                if len(up):
                    viol.append("A: stored above computed, tier %s set %d: %s" % (R.TIERS[tier], bset, up[:3]))
                tn = R.TIERS[tier]
                nz = a > 0
                if nz.any():
                    stats[tn]["max_stored_over_A"] = max(stats[tn]["max_stored_over_A"], float((s["stored"][nz] / a[nz]).max()))
        s = body[(body["tier"] == R.T_ROT) & (body["kind"] == R.K_FORM)]
        a = ex.rotation_bound()[s["block"], s["part"]]
        if (s["computed"] > a).any() or (s["stored"] > s["computed"]).any():
            viol.append("A: rotation bound above the exact bound: %s" % s[(s["computed"] > a) | (s["stored"] > s["computed"])][:3])
        if (a > 0).any():
            stats["rot"]["max_stored_over_A"] = float((s["stored"][a > 0] / a[a > 0]).max())
        # the bound part of a probe: the plain bound of the subsets that were not probed (word 9), no static alpha error
        s = body[body["tier"] == R.T_PROBE_FULL]
        for bset in (0, 1, 2):
            q = s[s["set"] == bset]
            if not len(q):
                continue
            g = ex.subsets((0, 1, 2, 3) if bset == 0 else (0, 1, 2), 3 if bset == 2 else 2)[q["block"], q["part"]]
            rest = g.sum(1) - g[np.arange(len(q)), q["sub"]]
            if (q["x"][:, 1] > rest).any() or (q["computed"].astype(np.float64) > q["x"][:, 0].astype(np.float64) + q["x"][:, 1].astype(np.float64)).any():
                viol.append("A: bound of the rest of a probe above the exact bound, set %d: %s" % (bset, q[q["x"][:, 1] > rest][:3]))
            if (rest > 0).any():
                stats["probe-full"]["max_stored_over_A"] = max(stats["probe-full"]["max_stored_over_A"], float((q["x"][:, 1][rest > 0] / rest[rest > 0]).max()))
        # sharp bounds: subset by subset with the recorded direction, then the sums
        subs = rec[rec["kind"] == R.K_SUBSET]
        per_part = {}
        for r in subs:
            key = (name if name != "hand_over" else "default", int(r["set"]), int(r["bits"]), int(r["block"]), int(r["part"]), int(r["sub"]), r["x"].tobytes())
            ref = _sharp_ref(key, blocks, ex, r)
            if float(r["computed"]) > ref:
                viol.append("A: sharp bound of a subset above the reference: %s (reference %r)" % (r, ref))
            per_part[(int(r["tier"]), int(r["set"]), int(r["bits"]), int(r["block"]), int(r["part"]), int(r["sub"]))] = ref
        for tier in (R.T_SHARP, R.T_PROBE_SHARP):
            for r in body[(body["tier"] == tier) & (body["kind"] == R.K_FORM_CMP)]:
                ns = int(r["subsets"])
                refs = [per_part.get((tier, int(r["set"]), int(r["bits"]), int(r["block"]), int(r["part"]), sub)) for sub in range(ns)]
                if tier == R.T_PROBE_SHARP:
                    refs[int(r["sub"])] = 0.0
                    value, extra = float(r["x"][1]), 0.0
                else:
                    value, extra = float(r["computed"]), (0.0 if r["set"] == 0 else ex.static[int(r["block"])])
                if any(x is None for x in refs):
                    viol.append("A: a sharp bound without its subset records: %s" % r)
                    continue
                a = sum(refs) + extra
                if value > a:
                    viol.append("A: sharp bound above the sum of its subsets' references: %s (reference %r)" % (r, a))
                if a > 0:
                    tn = R.TIERS[tier]
                    stats[tn]["max_stored_over_A"] = max(stats[tn]["max_stored_over_A"], value / a)
                if tier == R.T_SHARP:  # (the table keeps the largest value computed for the entry so far)
                    tab = prior[int(r["set"])]
                    tab[int(r["block"]), int(r["part"])] = max(tab[int(r["block"]), int(r["part"])], r["computed"])
                    if r["stored"] > tab[int(r["block"]), int(r["part"])]:
                        viol.append("A: stored above every value computed for the entry, sharp tier: %s" % r)

    # ---- reference B
    emat = {}
    for (m, w), (e, ok, _) in E.items():
        emat.setdefault(m, {})[w] = e
    for t, tname in enumerate(R.TIERS):
        sel = body[body["tier"] == t]
        if not len(sel):
            continue
        # the records of a tier fall into few (kind, set, bits, mode) groups; within one the candidates are (mode, partition)
        keys = np.stack([sel["kind"], sel["set"], sel["bits"], sel["mode"]], 1)
        for key in np.unique(keys, axis=0):
            q = sel[(keys == key).all(1)]
            for part in np.unique(q["part"]):
                qq = q[q["part"] == part]
                for (m, w) in _modes_held(qq[0]):
                    cls = in_class(m)[qq["block"]]
                    stats[tname]["pairs_out_of_class"] += int((~cls).sum())
                    qc = qq[cls]
                    if not len(qc):
                        continue
                    e = emat[m][w][qc["block"]]
                    val = np.maximum(qc["stored"], qc["computed"]).astype(np.float64)
                    stats[tname]["pairs_B"] += int(len(qc))
                    over = val > e * TOL_B
                    if over.any():
                        viol.append("B: %s value above the error the reference reaches for mode %d candidate %d: %s (E %s)" % (tname, m, w, qc[over][:3], e[over][:3]))
                    pos = e > 0
                    if pos.any():
                        h = float(((e[pos] - val[pos]) / e[pos]).min())
                        cur = stats[tname]["min_headroom_B"]
                        stats[tname]["min_headroom_B"] = h if cur is None else min(cur, h)
    assert not viol, "%s: %d violations\n%s" % (job, len(viol), "\n".join(viol[:12]))

    # the first-tier table: a record for every (block, bound set the wave computes, partition)
    t1 = body[(body["tier"] == R.T_TIER1) & (body["kind"] == R.K_FORM_CMP)]
    have = np.zeros((n, 3, 64), np.int64)
    np.add.at(have, (t1["block"], t1["set"], t1["part"]), 1)
    translucent = blocks[:, :, 3].min(1) < 255
    allowed = R.rgb_modes_allowed(blocks)
    for w0 in range(0, n, 16):
        wave = slice(w0, min(w0 + 16, n))
        # (the wave loads whole groups: blocks past n are read from block 0 and count for the group-wide booleans)
        full = np.arange(w0, w0 + 16)
        src = np.where(full < n, full, 0)
        any_alpha, any_rgb = translucent[src].any(), R.rgb_modes_allowed(blocks[src]).any()
        want = [bool(any_alpha), bool(any_rgb or not any_alpha), bool(any_rgb)]
        for bset in range(3):
            got = have[wave, bset]
            assert (got == (1 if want[bset] else 0)).all(), "%s: first-tier records of set %d in the wave at block %d: %s, expected %d each" % (
                job, bset, w0, np.unique(got), want[bset])
    return stats


@functools.lru_cache(maxsize=None)
def _analysed(name, n, dump_id):
    return analyse(name, n, _DUMPS[dump_id])


_DUMPS = {}


def analysed(name, n, dump):
    _DUMPS[id(dump)] = dump
    return _analysed(name, n, id(dump))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OPTION_SETS))
def test_bounds_of_the_kernel_are_sound(dump, name):
    """references A and B over every record of the three sizes, no overflow, the oracle's bytes, the first-tier table complete"""
    for n in SIZES:
        analysed(name, n, dump)


@pytest.mark.gpu
def test_every_tier_is_reached_and_report(dump):
    """so that the tests above cannot pass empty: over the union of the runs every tier has a record with a non-zero stored
    value and one that dropped a candidate.  Writes the figures the next change to the bounds will be argued with."""
    coverage_and_report(dump, REPORT)


def coverage_and_report(dump, path):
    report = {name: {str(n): analysed(name, n, dump) for n in SIZES} for name in OPTION_SETS}
    for tname in R.TIERS:
        nonzero = sum(report[o][s][tname]["nonzero"] for o in report for s in report[o])
        dropped = sum(report[o][s][tname]["dropped"] for o in report for s in report[o])
        assert nonzero > 0, "no %s record with a non-zero stored value" % tname
        assert dropped > 0, "no %s record that dropped a candidate" % tname
    hard = sum(int((np.ascontiguousarray(dump["records_hand_over_%d" % n]).view(R.RECORD_DTYPE)["hard"] != 0).sum()) for n in SIZES)
    assert hard > 0, "the forced hand-over handed nothing over"
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump({"tolerance_B": "E * (1 + 20 * 2^-24)", "hand_over_final_records": hard, "runs": report}, f, indent=1, sort_keys=True)
    return report
