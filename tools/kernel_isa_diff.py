#!/usr/bin/env python3
"""Proves that a source-only change left the device code alone: kernel by kernel, OLD_TREE against NEW_TREE.

    tools/kernel_isa_diff.py OLD_TREE NEW_TREE [-j JOBS] [-v]

Every priblast_amd/csrc/*.hip of both trees is compiled to device assembly with the command its own Makefile
would run (taken from `make --dry-run --always-make`), `-c` replaced by `--cuda-device-only -S`.  The assembly
is cut into functions; what depends only on a function's position in its file - the function index in local
labels such as .LBB<n>_<m> - is normalised away.  For every kernel of OLD_TREE the report says whether NEW_TREE
has a kernel of the same symbol name, in whichever file, with the same instruction stream and the same
.amdhsa_ descriptor (registers, LDS, scratch and the rest).  A kernel whose symbol is gone counts as "renamed" when
a kernel that only NEW_TREE has is the same instruction stream and descriptor; the pair is printed, old name to new.
Device functions that were not inlined are compared like the kernels.  Exit status 1 on any difference or missing
symbol.  Needs hipcc, no GPU.
"""
import argparse
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile

CSRC = os.path.join("priblast_amd", "csrc")
FIGURES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def compile_commands(tree):
    """{file.hip: argv} as the tree's Makefile compiles its HIP sources"""
    out = subprocess.run(["make", "-C", os.path.join(tree, CSRC), "--dry-run", "--always-make", "--no-print-directory", "all"],
                         check=True, capture_output=True, text=True).stdout
    cmds = {}
    for line in out.splitlines():
        argv = shlex.split(line)
        if "-c" in argv and "-o" in argv:
            src = argv[argv.index("-c") + 1]
            if src.endswith(".hip"):
                cmds[os.path.basename(src)] = argv
    if not cmds:
        sys.exit(f"{tree}: the Makefile's dry run shows no HIP compile command")
    return cmds


def device_asm(argv, tmpdir, tag):
    src = argv[argv.index("-c") + 1]
    dst = os.path.join(tmpdir, f"{tag}_{os.path.basename(src)}.s")
    cmd = []
    skip = False
    for a in argv:
        if skip:
            skip = False
        elif a == "-o":
            skip = True
        elif a == "-c":
            cmd += ["--cuda-device-only", "-S"]
        else:
            cmd.append(a)
    subprocess.run(cmd + ["-o", dst], check=True)
    with open(dst) as f:
        return f.read()


LOCAL = re.compile(r"\.L(BB|JTI|CPI|tmp|func_begin|func_end)\d+")


def normal(line):
    line = line.split(";", 1)[0].strip()
    return LOCAL.sub(r".L\1", line)


def split_asm(text):
    """-> ({symbol: [instruction lines]}, {kernel symbol: [descriptor lines]})"""
    funcs, descs = {}, {}
    is_func = set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    func = desc = None  # the function / the descriptor (which lies inside its kernel's function) being read
    for raw in text.splitlines():
        s = normal(raw)
        if not s:
            continue
        if func is None:
            if s.endswith(":") and s[:-1] in is_func:
                func = s[:-1]
                funcs[func] = []
        elif s.startswith(".amdhsa_kernel "):
            desc = s.split()[1]
            descs[desc] = []
        elif s == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            descs[desc].append(s)
        elif s.startswith(".Lfunc_end"):
            func = None
        else:
            funcs[func].append(s)
    return funcs, descs


def tree_code(tree, tmpdir, tag, jobs):
    """{symbol: {file: (instructions, descriptor or None)}}: a template kernel of a library may be in several files"""
    cmds = compile_commands(tree)
    code = {}
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        texts = ex.map(lambda name: device_asm(cmds[name], tmpdir, tag), sorted(cmds))
        for name, text in zip(sorted(cmds), texts):
            f, d = split_asm(text)
            for sym, body in f.items():
                code.setdefault(sym, {})[name] = (tuple(body), tuple(d[sym]) if sym in d else None)
    return code


def figures(desc):
    got = {}
    for line in desc or ():
        m = re.match(r"\.amdhsa_(\w+)\s+(.*)", line)
        if m and m.group(1) in FIGURES:
            got[m.group(1)] = m.group(2)
    return ", ".join(f"{k}={got[k]}" for k in FIGURES if k in got)


def demangle(syms):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(syms, out))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("-j", "--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("-v", "--verbose", action="store_true", help="list the identical kernels too")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = tree_code(a.old_tree, tmp, "old", a.jobs)
        new = tree_code(a.new_tree, tmp, "new", a.jobs)
    names = demangle(sorted(set(old) | set(new)))
    files = lambda variants: ",".join(sorted(variants)) if variants else "-"
    is_kernel = lambda variants: any(desc is not None for _, desc in variants.values())
    # a kernel that only NEW_TREE has, by what it is - its versions with its own symbol (a directive may name it) taken
    # out -: the code of an old kernel under another name
    nameless = lambda sym, variants: frozenset((tuple(line.replace(sym, "@") for line in c), d) for c, d in variants.values())
    only_new = {}
    for s in sorted(set(new) - set(old), key=lambda s: names[s]):
        if is_kernel(new[s]):
            only_new.setdefault(nameless(s, new[s]), []).append(s)
    bad = 0
    renamed = set()
    for sym in sorted(old, key=lambda s: (files(old[s]), names[s])):
        o, n = old[sym], new.get(sym, {})
        if not n and is_kernel(o) and nameless(sym, o) in only_new:
            same = only_new[nameless(sym, o)]  # (several of one code: each taken once, while they last)
            to = same.pop(0) if len(same) > 1 else same[0]
            renamed.add(to)
            print(f"{'renamed':10s} {'kernel':8s} {files(o)} -> {files(new[to])}: {names[sym]} -> {names[to]}")
            continue
        if not n:
            verdict = "MISSING"
        else:  # the same versions of the code (one, unless the copies of a library's kernel differ between files)
            same_code = {c for c, _ in o.values()} == {c for c, _ in n.values()}
            same_desc = {d for _, d in o.values()} == {d for _, d in n.values()}
            verdict = "identical" if same_code and same_desc else "DIFFERS in " + " and ".join(
                w for w, ok in (("instructions", same_code), ("descriptor", same_desc)) if not ok)
        if verdict != "identical":
            bad += 1
        if verdict != "identical" or a.verbose:
            print(f"{verdict:10s} {'kernel' if is_kernel(o) else 'function':8s} {files(o)} -> {files(n)}: {names[sym]}")
            if verdict.startswith("DIFFERS"):
                for tag, variants in (("old", o), ("new", n)):
                    for name, (c, d) in sorted(variants.items()):
                        print(f"           {tag} {name}: {len(c)} lines, {figures(d)}")
    added = sorted(set(new) - set(old) - renamed)
    for sym in added:
        print(f"{'new':10s} {'kernel' if is_kernel(new[sym]) else 'function':8s} - -> {files(new[sym])}: {names[sym]}")
    kernels = sum(1 for s in old if is_kernel(old[s]))
    print(f"{kernels} kernels and {len(old) - kernels} device functions of {a.old_tree}: {len(old) - bad - len(renamed)} identical in {a.new_tree}, "
          f"{len(renamed)} renamed, {bad} different or missing; {len(added)} only in {a.new_tree}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
