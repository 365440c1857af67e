"""csrc/hip_owned.h, the move-only owners of what the shim allocates through the HIP runtime, on the CPU over counting stand-ins
for the hip* calls (tests/hip_owned_harness.cpp), under AddressSanitizer and UndefinedBehaviorSanitizer: every allocation freed
exactly once after moves, regrowth and scope exit; a smaller reserve allocates nothing; a failing allocation leaves the owner
empty and usable; the owners do not copy (static_assert); a half-built struct of owners frees what exists and nothing else."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = tmp_path_factory.mktemp("hip_owned") / "harness"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "hip_owned_harness.cpp"), "-o", str(exe)]
    try:
        # can the compiler do that at all?  (only then is a harness that does not compile a failure)
        probe = subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", str(exe) + "_probe"],
                               input=b"int main() { return 0; }\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    except OSError:
        pytest.skip("g++ not usable here")
    if probe.returncode != 0:
        pytest.skip("g++ -fsanitize=address,undefined not usable here")
    subprocess.check_call(cmd)
    return str(exe)


def test_owners_under_sanitizers(harness):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([harness], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    out = p.stdout.decode() + p.stderr.decode()
    assert p.returncode == 0 and out.startswith("ok "), out[-3000:]
