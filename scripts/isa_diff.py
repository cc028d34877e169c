#!/usr/bin/env python3
"""Which kernels does a change to csrc/ touch?  Compiles every *_kernels.hip of two csrc directories to gfx950 assembly
(device only, the flags csrc/Makefile of that side gives the file) and compares them kernel by kernel:
    python scripts/isa_diff.py <csrc dir A> <csrc dir B> [--diag]        (--diag: the diagnostic library, -DIAS_DIAG)
Kernels are matched by symbol across all files of a side, so one that moved to another file is compared like any other
(and listed as moved); reported under the file B has it in: the kernels only A or only B has, the number whose code is
identical, and for every kernel that differs the VGPR / SGPR / scratch / LDS figures of both sides from the code objects'
metadata and whether the multiset of its instruction mnemonics is equal (then only registers or the order differ).  A
kernel's text is its function (from its `.type ...,@function` to the `.Lfunc_end` label) and its `.amdhsa_kernel`
descriptor, without comments and with the function index taken out of the local labels (.LBB<n>_<k>), which shifts
whenever a kernel in front of it comes or goes.
Exit status 1 if a kernel both sides have differs.  Needs hipcc only (no GPU)."""
import argparse
import collections
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIGURES = (("vgpr_count", "VGPR"), ("agpr_count", "AGPR"), ("sgpr_count", "SGPR"), ("private_segment_fixed_size", "scratch B"),
           ("group_segment_fixed_size", "LDS B"))


def makefile_flags(csrc):
    """(flags of every file, {file: its extra flags}) as csrc/Makefile states them"""
    text = open(os.path.join(csrc, "Makefile")).read()
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    base = re.search(r"^HIPFLAGS\s*=\s*(.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()
    extra = {}
    # one list of files and their flag as a target-specific variable: `$(LIST:%=%.o) ...: FILEFLAGS = <flags>`
    for var, flags in re.findall(r"^\$\((\w+):%=%\.o\).*:\s*\w+\s*\+?=\s*(.*)$", text, re.M):
        for stem in re.search(rf"^{var}\s*=\s*(.*)$", text, re.M).group(1).split():
            extra[stem + ".hip"] = flags.split()
    # trees before that: a rule of its own per such file
    for stem, recipe in re.findall(r"^(\w+)\.o:.*\n\t(.*)$", text, re.M):
        words = recipe.split()
        extra[stem + ".hip"] = [w for w in words if w.startswith("-f") and w not in base]
    return base, extra


def compile_asm(csrc, src, diag, out):
    base, extra = makefile_flags(csrc)
    cmd = [HIPCC] + base + extra.get(src, []) + (["-DIAS_DIAG"] if diag else []) + ["-S", "--cuda-device-only", src, "-o", out]
    r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} (in {csrc}) failed:\n{r.stdout}")
    return open(out).read()


def normalise(text):
    lines = []
    for l in text.split("\n"):
        l = l.split(";", 1)[0].rstrip()
        if l:
            lines.append(re.sub(r"(\.L[A-Za-z_]+?)\d+(_\d+|\b)", r"\1\2", l))
    return "\n".join(lines)


def kernels_of(asm):
    """{symbol: (normalised text, {figure: value})} of every function of an assembly file"""
    meta = {}
    cur = None
    m = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", asm, re.M | re.S)
    for l in (m.group(1) if m else "").split("\n"):
        k = re.match(r"^(  - |    )\.(\w+):\s*(\S+)\s*$", l)
        if not k:
            continue
        if k.group(1) == "  - ":
            cur = {}
        cur[k.group(2)] = k.group(3)
        if k.group(2) == "name":
            meta[k.group(3)] = cur
    desc = {m.group(1): m.group(0) for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel", asm, re.M | re.S)}
    out = {}
    for m in re.finditer(r"^\t\.type\t(\S+),@function\n", asm, re.M):
        sym = m.group(1)
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(asm, m.end())
        if end is None:
            raise SystemExit(f"no .Lfunc_end after {sym}")
        out[sym] = (normalise(asm[m.end():end.start()] + "\n" + desc.get(sym, "")), meta.get(sym, {}))
    return out


def mnemonics(text):
    """Counter of the instruction mnemonics of a kernel's normalised text (labels and directives left out)"""
    c = collections.Counter()
    for l in text.split("\n"):
        t = l.strip()
        if l.startswith("\t") and t and t[0] != "." and not t.endswith(":"):
            c[t.split()[0]] += 1
    return c


def demangle(names):
    tool = shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    r = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True)
    return dict(zip(names, r.stdout.split("\n")))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--diag", action="store_true", help="compile with -DIAS_DIAG (libias_hip_diag.so)")
    ap.add_argument("--jobs", type=int, default=16)
    args = ap.parse_args()
    dirs = [os.path.abspath(args.a), os.path.abspath(args.b)]
    files = sorted({os.path.basename(p) for d in dirs for p in glob.glob(os.path.join(d, "*_kernels.hip"))})
    with tempfile.TemporaryDirectory() as td, concurrent.futures.ThreadPoolExecutor(max(1, min(args.jobs, 16))) as pool:
        jobs = {(f, i): pool.submit(compile_asm, d, f, args.diag, os.path.join(td, f"{i}_{f}.s"))
                for f in files for i, d in enumerate(dirs) if os.path.exists(os.path.join(d, f))}
        sides = [{}, {}]                                   # symbol -> (file, text, figures)
        for (f, i), job in sorted(jobs.items()):
            for sym, (text, figs) in kernels_of(job.result()).items():
                sides[i][sym] = (f, text, figs)
        ka, kb = sides
        total = {"only_a": 0, "only_b": 0, "same": 0, "diff": 0, "moved": 0}
        for f in files:
            only_a = sorted(k for k in ka if k not in kb and ka[k][0] == f)
            only_b = sorted(k for k in kb if k not in ka and kb[k][0] == f)
            both = sorted(k for k in kb if k in ka and kb[k][0] == f)
            diff = [k for k in both if ka[k][1] != kb[k][1]]
            moved = [k for k in both if ka[k][0] != f]
            name = demangle(only_a + only_b + diff + moved)
            print(f"{f}: {len(both) - len(diff)} identical, {len(diff)} different, {len(only_a)} only in A, {len(only_b)} only in B"
                  + (f", {len(moved)} moved here" if moved else ""))
            for k in only_a:
                print(f"  only in A: {name[k]}")
            for k in only_b:
                print(f"  only in B: {name[k]}")
            for k in moved:
                print(f"  moved from {ka[k][0]} ({'DIFFERENT' if k in diff else 'identical'}): {name[k]}")
            for k in diff:
                figs = ", ".join(f"{label} {ka[k][2].get(key, '?')} -> {kb[k][2].get(key, '?')}" for key, label in FIGURES)
                ma, mb = mnemonics(ka[k][1]), mnemonics(kb[k][1])
                mn = "mnemonic multiset equal" if ma == mb else \
                    "mnemonic multiset DIFFERS (" + ", ".join(f"{m} {ma[m]} -> {mb[m]}" for m in sorted(set(ma) | set(mb)) if ma[m] != mb[m]) + ")"
                print(f"  DIFFERENT: {name[k]}: {figs}; {ka[k][1].count(chr(10)) + 1} -> {kb[k][1].count(chr(10)) + 1} lines; {mn}")
            total["only_a"] += len(only_a); total["only_b"] += len(only_b); total["moved"] += len(moved)
            total["same"] += len(both) - len(diff); total["diff"] += len(diff)
    print(f"total: {total['same']} identical, {total['diff']} different, {total['only_a']} only in A, {total['only_b']} only in B, "
          f"{total['moved']} moved")
    return 1 if total["diff"] else 0


if __name__ == "__main__":
    sys.exit(main())
