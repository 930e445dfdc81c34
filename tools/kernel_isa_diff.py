#!/usr/bin/env python3
"""Did a source change touch the machine code of a kernel that it kept?  Needs hipcc, no GPU.

    python tools/kernel_isa_diff.py compile <tree> <out dir>     every csrc/*.hip of <tree>, both flavours,
                                                                 device-only to gfx950 assembly
    python tools/kernel_isa_diff.py compare <parent dir> <change dir> [--drop REGEX=REPL ...]

compare lists the kernels (.amdhsa_kernel) of each file on both sides and, for every kernel present on
both, compares the body from its label to its end and its .amdhsa_ resource directives.  Normalised
first: the kernel's own mangled name, comments, and the index of the function inside its file that
local labels carry (.LBB<n>_<m>).  --drop rewrites parent names whose template arguments the change
removed, e.g. --drop 'k_linear_dmaILi0E(Li\\d+ELi\\d+EE)=k_linear_dmaI\\1'.  (profiles/r07_kernel_set_isa.txt)"""
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def compile_tree(tree, out):
    from rag_fin_amd import build
    os.makedirs(out, exist_ok=True)
    jobs = []
    for src in sorted(glob.glob(os.path.join(tree, "rag_fin_amd", "csrc", "*.hip"))):
        for flavour, extra in (("prod", []), ("exp", ["-DRF_EXPERIMENTS"])):
            dst = os.path.join(out, os.path.basename(src)[:-4] + "." + flavour + ".s")
            jobs.append([build._hipcc(), *build.FLAGS, *extra, "--cuda-device-only", "-S", src, "-o", dst])
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        for r in ex.map(lambda c: subprocess.run(c, capture_output=True, text=True), jobs):
            if r.returncode != 0:
                sys.exit(r.stderr)


def kernels(path):
    """mangled name -> (body, resource directives), normalised"""
    txt = open(path).read()
    res = {}
    for n in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, flags=re.M):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\t\.section\t\.rodata" % re.escape(n), txt, flags=re.M | re.S).group(1)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+%s\n(.*?)^\s*\.end_amdhsa_kernel" % re.escape(n), txt, flags=re.M | re.S).group(1)
        body = re.sub(r"[ \t]*;[^\n]*", "", body.replace(n, "<KERNEL>"))
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        res[n] = ("\n".join(l for l in body.split("\n") if l.strip()), desc.replace(n, "<KERNEL>"))
    return res


def compare(pdir, cdir, drops):
    def renamed(n):
        for pat, repl in drops:
            n = re.sub(pat, repl, n)
        return n
    differing = 0
    for f in sorted(glob.glob(os.path.join(pdir, "*.s"))):
        base = os.path.basename(f)
        P = {renamed(n): v for n, v in kernels(f).items()}
        C = kernels(os.path.join(cdir, base))
        both = sorted(set(P) & set(C))
        diff = [k for k in both if P[k] != C[k]]
        differing += len(diff)
        print("%s: parent %d kernels, change %d, in both %d, differing %d" % (base, len(P), len(C), len(both), len(diff)))
        for tag, names in (("DIFFERS", diff), ("only in parent", sorted(set(P) - set(C))), ("only in change", sorted(set(C) - set(P)))):
            for k in names:
                print("    %s: %s" % (tag, k))
    print("RESULT: %d kernels present on both sides differ" % differing)
    return differing


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "compile":
        compile_tree(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        drops = [tuple(a.split("=", 1)) for a in sys.argv[5:]] if sys.argv[4:5] == ["--drop"] else []
        sys.exit(1 if compare(sys.argv[2], sys.argv[3], drops) else 0)
    else:
        sys.exit(__doc__)
