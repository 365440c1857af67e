"""The C++ face (include/cvtt/ConvectionKernels.h, csrc/cxx_api.cpp, coalescer.h) held to the reference's own bytes by ONE
client program of cvtt::Kernels, oracle/dropin_client.cpp, compiled twice from the same source:

  oracle/_ref/dropin_client_ref   against the reference's header and sources (oracle/Makefile, target `ref`), and
  <tmp>/dropin_client             against our header and libcvtt_mi355x.so (here, once per module).

Both run on the same box, section by section, and must print the same lines: every one-group entry over 8 content groups x 6
option sets, BC7 over 5 plans, the ETC forms with scratch allocated under the call's own and under other Options, the three
decoders on encoder output and on forced mode / header bits, every *Batch entry against the reference's one-group loop, and
16 caller threads of 13 kinds that differ from a base call in one thing each (the coalescer's key).  The `host` section needs
no device: signatures (a table of function pointers of the reference's types), constructors, flag values, plans.

CPU: our build compiles; `host` is identical.  GPU: one test per section.
"""
import hashlib
import os
import subprocess
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "oracle", "dropin_client.cpp")
REF_EXE = os.path.join(ROOT, "oracle", "_ref", "dropin_client_ref")
GPU_SECTIONS = ("s3tc", "bc7", "bc6h", "etc", "eac", "decode", "batch", "threads")
THREAD_REPETITIONS = 30  # ours; the reference runs each thread's calls once
TIME_LIMIT = 120  # seconds per program run; a section takes a few seconds at the most


def _source_sha():
    with open(SOURCE, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


@pytest.fixture(scope="module")
def our_exe(tmp_path_factory):
    """oracle/dropin_client.cpp against our header and library, as test_abi._build_cxx_client builds its client"""
    from convectionkernels_amd import api
    exe = tmp_path_factory.mktemp("dropin") / "dropin_client"
    libdir = os.path.dirname(os.path.abspath(os.environ.get("CVTTMI_LIB", api._LIB_PATH)))
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-pthread", "-I", os.path.join(ROOT, "include", "cvtt"),
                           "-DCLIENT_SRC_SHA=" + _source_sha(), SOURCE, "-o", str(exe),
                           "-L", libdir, "-lcvtt_mi355x", "-Wl,-rpath," + libdir], timeout=300)
    return str(exe)


@pytest.fixture(scope="module")
def ref_exe():
    if not os.path.exists(REF_EXE):
        pytest.skip("oracle/_ref/dropin_client_ref not present")
    return REF_EXE


def _run(exe, section, repetitions=1):
    """one section of one program under its own time limit -> (lines after the hash line, seconds)"""
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(TIME_LIMIT), exe, section, str(repetitions)],
                       capture_output=True, text=True, timeout=TIME_LIMIT + 30)
    seconds = time.time() - t0
    assert p.returncode == 0, "%s %s: exit status %d\n%s" % (os.path.basename(exe), section, p.returncode, p.stderr[-2000:])
    lines = p.stdout.splitlines()
    assert lines and lines[0].startswith("source_sha "), lines[:1]
    return lines[0].split()[1], lines[1:], seconds


def _key(line):
    return " ".join(line.split(" ")[:4])  # section, entry, option set, group


def differences(ref_lines, our_lines):
    """[(key, what)] for every line that is not the same in both outputs; keys are compared in the reference's order"""
    ours = {}
    for l in our_lines:
        ours.setdefault(_key(l), []).append(l)
    diffs = []
    seen = set()
    for l in ref_lines:
        k = _key(l)
        seen.add(k)
        got = ours.get(k)
        if not got:
            diffs.append((k, "missing from our output"))
        elif got.pop(0) != l:
            diffs.append((k, "differs"))
    for k, rest in ours.items():
        if rest:
            diffs.append((k, "only in our output" if k not in seen else "printed more often by ours"))
    if not diffs and ref_lines != our_lines:
        diffs.append((_key(our_lines[0]) if our_lines else "-", "same lines in another order"))
    return diffs


def compare_section(ref_exe, our_exe, section, our_repetitions=1):
    sha = _source_sha()
    ref_sha, ref_lines, ref_s = _run(ref_exe, section)
    assert ref_sha == sha, ("oracle/_ref/dropin_client_ref was built from another oracle/dropin_client.cpp (%s, now %s): "
                            "rebuild oracle/_ref (make -C oracle ref)" % (ref_sha[:12], sha[:12]))
    our_sha, our_lines, our_s = _run(our_exe, section, our_repetitions)
    assert our_sha == sha
    print("section %s: reference %.2f s (%d lines), ours %.2f s" % (section, ref_s, len(ref_lines), our_s))
    assert len(ref_lines) > 3, ref_lines
    diffs = differences(ref_lines, our_lines)
    assert not diffs, ("section %s: %d of %d lines differ from the reference's; first: %s"
                       % (section, len(diffs), len(ref_lines), "; ".join("%s (%s)" % d for d in diffs[:5])))
    return ref_lines, our_lines


def test_differences_names_keys():
    """the comparison itself: a changed, a missing and an extra line are each reported by their key"""
    ref = ["s3tc EncodeBC4U default noise 00", "s3tc EncodeBC4S default noise 11", "s3tc EncodeBC5U default noise 22"]
    assert differences(ref, list(ref)) == []
    assert differences(ref, [ref[0], "s3tc EncodeBC4S default noise 12", ref[2]]) == [("s3tc EncodeBC4S default noise", "differs")]
    assert differences(ref, ref[:2]) == [("s3tc EncodeBC5U default noise", "missing from our output")]
    assert differences(ref, ref + ["s3tc EncodeBC1 default noise 33"]) == [("s3tc EncodeBC1 default noise", "only in our output")]
    assert differences(ref, [ref[1], ref[0], ref[2]]) == [("s3tc EncodeBC4S default noise", "same lines in another order")]


def test_client_compiles_against_our_header(our_exe):
    """every entry point of the reference, assigned to a function pointer of the reference's own type, exists in our header
    with that type (a drifted signature is a compile error), and the program links against the library"""
    p = subprocess.run(["timeout", "-k", "10", "60", our_exe], capture_output=True, text=True, timeout=90)
    assert p.returncode == 2 and p.stdout.split() == ["source_sha", _source_sha()], (p.returncode, p.stdout, p.stderr)


def test_host_section_is_the_references(ref_exe, our_exe):
    """no device: sizeof and bytes of the default-constructed PODs, every Flags enumerator, NumParallelBlocks, plans from ten
    qualities (below, at and above the clamps) and from four fine-tuning sets with the return value"""
    ref_lines, _ = compare_section(ref_exe, our_exe, "host")
    entries = {l.split()[1] for l in ref_lines}
    assert {"signatures", "sizeof", "default", "flag", "plan_from_quality", "plan_from_fine_tuning"} <= entries


@pytest.mark.gpu
@pytest.mark.parametrize("section", GPU_SECTIONS)
def test_section_equals_reference(gpu_ctx, ref_exe, our_exe, section):
    """both programs exit with status 0 and print the same lines; `threads` (ours with 30 repetitions per thread) also needs
    every thread to have got its first result again in every repetition"""
    ref_lines, our_lines = compare_section(ref_exe, our_exe, section, THREAD_REPETITIONS if section == "threads" else 1)
    if section == "threads":
        counts = [l.split() for l in our_lines if l.split()[1] == "differing_repetitions"]
        assert len(counts) == 16, counts
        unstable = [(c[2], c[3], c[4]) for c in counts if c[4] != "0"]
        assert not unstable, "threads whose repetitions differed from their first result (kind, thread, repetitions): %s" % unstable
        assert len({l.split()[2] for l in our_lines if l.split()[1] == "final"}) == 13  # every kind ran
    if section in ("etc", "batch", "threads"):
        release = [l.split() for l in our_lines if l.split()[1] == "Release"]
        assert release and all(r[4] == "0" for r in release), release
