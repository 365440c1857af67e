#!/usr/bin/env python3
"""Are the kernels of two builds of the library the same instructions?  (developer tool, no GPU needed)
   python tools/isa_identity.py [--rename REGEX=TEXT]... [--gone REGEX] parent/libcvtt_mi355x.so [lib.so]
Disassembles the gfx950 code objects of both libraries (kernel_resources.code_objects, llvm-objdump -d) and compares kernel
by kernel: the instruction stream without addresses, and the register / LDS / scratch figures of the metadata.  For a kernel
that differs it prints the instruction counts and the histogram of mnemonics that changed.  Exit status 1 if any differs.
--rename: the first library's kernel names are compared under re.sub(REGEX, TEXT), for a change that only renames kernels; given
more than once, the maps are applied in the order given.
--gone: kernels of the first library that the change removes on purpose; they are listed and do not count as differing.  Both
are searched in every kernel's name, so they name the kernels they mean: dropping a trailing `true` of the mip kernels alone is
   --rename '^(cvttmi_(?:downsample|mipfilter|mipresample)\w*<.*), true>$=\1>' --gone '^cvttmi_(downsample|mipfilter|mipresample)\w*<.*, false>$'
(a bare ', true>=>' would rename cvttmi_bc1_kernel<false, true> as well).  The first line of the output is the command with the
two libraries named by their source SHA-256, so that a recorded comparison states its name map; the last says how many
pc-relative literals were left out of the comparison."""
import collections
import ctypes
import os
import re
import shlex
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_resources as kr

OBJDUMP = os.path.join(os.path.dirname(kr.READELF), "llvm-objdump")
MASKED = [0]  # literals that instructions() left out, over all its calls


def instructions(path):
    """{demangled kernel: [instruction text, ...]} of every function symbol in the library's code objects"""
    res = {}
    for obj in kr.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(obj)
            f.flush()
            txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "-C", f.name], capture_output=True, text=True, check=True).stdout
        cur, pc = None, set()
        for line in txt.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
            if m:
                name = re.sub(r"\(.*", "", m.group(1).replace("(anonymous namespace)::", "")).replace("void ", "")
                cur, pc = (None if name.startswith("__hip_cuid_") else res.setdefault(name, [])), set()
            elif cur is not None and line.startswith("\t"):
                # "\tv_add_f32 v1, v2, v3   // 000000001234: " -> the text; branch targets are relative, so position-free
                text = re.sub(r"\s+", " ", line.split("//")[0]).strip()
                # ... but the address of a constant table is the pc (s_getpc_b64 s[n:n+1]) plus its distance from there, a literal
                # that moves with everything linked in between: the s_add_u32 / s_addc_u32 that add it compare without it
                m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]$", text)
                if m:
                    pc = {"s" + m.group(1), "s" + m.group(2)}
                m = re.match(r"(s_addc?_u32 (s\d+), \2, )(0x[0-9a-f]+|\d+)$", text)
                if m and m.group(2) in pc:
                    pc.discard(m.group(2))
                    text = m.group(1) + "<distance>"
                    MASKED[0] += 1
                cur.append(text)
    # the zero bytes that align the next function are disassembled with the one before them ("..." for a run of them, a single
    # zero dword as the instruction it encodes); how many there are depends on the neighbours, not on the kernel
    for ins in res.values():
        while ins and ins[-1] in ("...", "v_cndmask_b32_e32 v0, s0, v0, vcc"):
            ins.pop()
    return res


def source_sha256(path):
    """the build identity compiled into a library (cvttmi_source_sha256), or "unknown" where it cannot be loaded"""
    try:
        sys.path.insert(0, kr.ROOT)
        from convectionkernels_amd import api
        api._preload_hip_runtime()
        fn = ctypes.CDLL(os.path.abspath(path)).cvttmi_source_sha256
        fn.restype = ctypes.c_char_p
        return (fn() or b"unknown").decode()
    except (OSError, AttributeError, ImportError):
        return "unknown"


def main():
    args = sys.argv[1:]
    renames, gone = [], None
    while args and args[0] in ("--rename", "--gone"):
        if args[0] == "--rename":
            renames.append(args[1].split("=", 1))
        else:
            gone = args[1]
        args = args[2:]
    options = sys.argv[1:len(sys.argv) - len(args)]
    a_path = args[0]
    b_path = args[1] if len(args) > 1 else os.path.join(kr.ROOT, "convectionkernels_amd", "lib", "libcvtt_mi355x.so")
    print("python tools/isa_identity.py %s <first: library of source SHA-256 %s> <second: library of source SHA-256 %s>"
          % (" ".join(shlex.quote(o) for o in options), source_sha256(a_path), source_sha256(b_path)))
    A, B = instructions(a_path), instructions(b_path)
    RA, RB = kr.kernels(a_path), kr.kernels(b_path)
    if gone:
        for k in sorted(k for k in A if re.search(gone, k)):
            print("%-72s %6d instructions  gone (only in the first, as stated)" % (k[:72], len(A.pop(k))))
    for regex, text in renames:
        A = {re.sub(regex, text, k): v for k, v in A.items()}
        RA = {re.sub(regex, text, k): v for k, v in RA.items()}
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
    print("%d kernels, %d differ (%d pc-relative literals of s_add_u32 / s_addc_u32 after s_getpc_b64 not compared)"
          % (len(set(A) | set(B)), differing, MASKED[0]))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
