#!/usr/bin/env python3
"""Per-kernel instruction listing of a gfx950 code object, for comparing two builds:   tools/kisa.py <file.o | file.hip> [more files]
One line per kernel: demangled name, instruction count, SHA-256 of the instruction text (addresses and encodings stripped, the alignment
fill behind the last s_endpgm dropped; branch operands are relative, so the text does not depend on where the kernel lands in .text)."""
import hashlib, os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "manhattanslam_amd", "csrc")
LLVM = "/opt/rocm/llvm/bin/"
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden -fno-gpu-flush-denormals-to-zero "
         "-I%s -I%s" % (CSRC, os.path.join(ROOT, "include"))).split()   # the Makefile's code generation flags


def kernels(path, tmp):
    """{kernel name: [instruction text, ...]} of the object (a .hip source is compiled first)."""
    run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout
    if path.endswith(".hip"):
        own = run("make", "-s", "-C", CSRC, "print-file-flags", "F=" + os.path.basename(path)[:-4]).split()   # what the Makefile adds for this file alone
        run("/opt/rocm/bin/hipcc", *FLAGS, *own, "-c", path, "-o", os.path.join(tmp, "k.o"))
        path = os.path.join(tmp, "k.o")
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "gfx950.co")
    run(LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, path, os.devnull)
    run(LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co)
    out, cur = {}, None
    for l in run(LLVM + "llvm-objdump", "-d", "--demangle", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(.*)>:$", l)
        if m: cur = out.setdefault(m.group(1), []); continue
        if cur is not None and l.startswith("\t"): cur.append(re.sub(r"\s+", " ", l.split("//")[0]).strip())
    for k, v in out.items():   # alignment fill behind the kernel's last s_endpgm differs with what follows it
        ends = [i for i, t in enumerate(v) if t.startswith("s_endpgm")]
        if ends: del v[ends[-1] + 1:]
    return {k: v for k, v in out.items() if v}


for f in sys.argv[1:]:
    with tempfile.TemporaryDirectory() as tmp:
        for name, ins in sorted(kernels(f, tmp).items()):
            print("%s  %6d  %s" % (hashlib.sha256("\n".join(ins).encode()).hexdigest(), len(ins), name))
