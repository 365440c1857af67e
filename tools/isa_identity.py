#!/usr/bin/env python3
"""Are the kernels of two builds of the library the same instructions?  (developer tool, no GPU needed)
   python tools/isa_identity.py parent/libcvtt_mi355x.so [lib.so]
Disassembles the gfx950 code objects of both libraries (kernel_resources.code_objects, llvm-objdump -d) and compares kernel
by kernel: the instruction stream without addresses, and the register / LDS / scratch figures of the metadata.  For a kernel
that differs it prints the instruction counts and the histogram of mnemonics that changed.  Exit status 1 if any differs."""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr

OBJDUMP = os.path.join(os.path.dirname(kr.READELF), "llvm-objdump")


def instructions(path):
    """{demangled kernel: [instruction text, ...]} of every function symbol in the library's code objects"""
    res = {}
    for obj in kr.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "-C", f.name], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                name = re.sub(r"\(.*", "", m.group(1).replace("(anonymous namespace)::", "")).replace("void ", "")
                cur = None if name.startswith("__hip_cuid_") else res.setdefault(name, [])
            elif cur is not None and line.startswith("\t"):
                # "\tv_add_f32 v1, v2, v3   // 000000001234: " -> the text; branch targets are relative, so position-free
                cur.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())
    return res


def main():
    args = sys.argv[1:]
    a_path = args[0]
    b_path = args[1] if len(args) > 1 else os.path.join(kr.ROOT, "convectionkernels_amd", "lib", "libcvtt_mi355x.so")
    A, B = instructions(a_path), instructions(b_path)
    RA, RB = kr.kernels(a_path), kr.kernels(b_path)
    differing = 0
    for k in sorted(set(A) | set(B)):
        if k not in A or k not in B:
            print("%-72s only in %s" % (k[:72], "the second" if k not in A else "the first"))
            differing += 1
            continue
        same = A[k] == B[k] and RA.get(k) == RB.get(k)
        print("%-72s %6d instructions  %s" % (k[:72], len(B[k]), "identical" if same else "DIFFERENT"))
        if same:
            continue
        differing += 1
        print("    instructions %d -> %d;  resources %s -> %s" % (len(A[k]), len(B[k]), RA.get(k), RB.get(k)))
        ha = collections.Counter(i.split(" ")[0] for i in A[k])
        hb = collections.Counter(i.split(" ")[0] for i in B[k])
        moved = {m: (ha[m], hb[m]) for m in sorted(set(ha) | set(hb)) if ha[m] != hb[m]}
        print("    mnemonic histogram: %s" % ("equal" if not moved else ", ".join("%s %d -> %d" % (m, x, y) for m, (x, y) in moved.items())))
        valu = lambda h: sum(n for m, n in h.items() if m.startswith("v_"))
        print("    VALU instructions %d -> %d" % (valu(ha), valu(hb)))
    print("%d kernels, %d differ" % (len(set(A) | set(B)), differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
