"""Compare the generated gfx950 code of two trees, kernel by kernel (hipcc cross-compiles: no GPU needed).  For a refactor that moves device code between files:

    python tools/kernel_asm_diff.py OLD/nrsc5_amd/csrc NEW/nrsc5_amd/csrc --a k_sync.hip --b k_sync.hip k_pids_px.hip

Every kernel symbol found on either side prints `same`, `DIFF` (with both instruction counts) or `MISSING`, followed by both sides' VGPR / SGPR / LDS / scratch
figures from -Rpass-analysis=kernel-resource-usage.  Text only: `.LBB<n>_` label numbers and trailing `;` comments are normalised away, nothing else is
interpreted.  The compile line and the function splitter are those of tests/test_codegen_guards.py.  Exit code 1 if any kernel is not `same`."""
import argparse
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_codegen_guards as guards  # noqa: E402

FIGURES = (("VGPR", r"VGPRs: (\d+)"), ("SGPR", r"SGPRs: (\d+)"), ("LDS", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"))


def _normal(ins):
    return [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", t)) for t in ins]


def kernels_of(csrc, sources):
    """kernel symbol -> (normalised instruction lines, resource figures, source file) for the listed .hip files of one tree"""
    csrc = os.path.abspath(csrc)
    include = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")
    guards.CSRC = csrc                                           # _asm compiles os.path.join(CSRC, source) with FLAGS
    guards.FLAGS = [f for f in guards.FLAGS if not f.startswith("-I")] + ["-I" + include, "-I" + csrc]
    out = {}
    for src in sources:
        asm, remarks = guards._asm(src)
        fns = guards._functions(asm)
        res = {b.split()[0]: b for b in remarks.split("Function Name: ")[1:]}
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M):
            assert name not in out, (name, "defined twice", src, out[name][2])
            fig = tuple(int(m.group(1)) if (m := re.search(pat, res.get(name, ""))) else -1 for _, pat in FIGURES)
            out[name] = (_normal(fns[name]), fig, src)
    return out


def _demangled(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not filt or not names:
        return {n: n for n in names}
    txt = subprocess.run([filt] + list(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"^void ", "", d).split("(")[0] for n, d in zip(names, txt)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("csrc_a")
    ap.add_argument("csrc_b")
    ap.add_argument("--a", nargs="+", required=True, metavar="HIP", help=".hip files of the first tree")
    ap.add_argument("--b", nargs="+", metavar="HIP", help=".hip files of the second tree (default: the same names)")
    args = ap.parse_args()
    A, B = kernels_of(args.csrc_a, args.a), kernels_of(args.csrc_b, args.b or args.a)
    names = sorted(set(A) | set(B))
    pretty = _demangled(names)
    print("# a: %s %s\n# b: %s %s\n# figures: %s" % (args.csrc_a, " ".join(args.a), args.csrc_b, " ".join(args.b or args.a), " / ".join(n for n, _ in FIGURES)))
    bad = 0
    for n in names:
        a, b = A.get(n), B.get(n)
        fig = lambda k: "%s %s" % (k[2], "/".join(map(str, k[1]))) if k else "-"
        if a is None or b is None:
            verdict = "MISSING in %s" % ("a" if a is None else "b")
        elif a[0] == b[0]:
            verdict = "same" if a[1] == b[1] else "DIFF in the figures only"
        else:
            verdict = "DIFF %d -> %d instructions" % tuple(sum(1 for t in k[0] if t and not t.endswith(":")) for k in (a, b))   # (labels and fences not counted)
        bad += verdict != "same"
        print("%-36s %-34s a: %-28s b: %s" % (pretty[n], verdict, fig(a), fig(b)))
    print("# %d kernels, %d not the same" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
