#!/usr/bin/env python3
"""Is the device code of two builds the same?  Compares two gfx950 assembly files (hipcc --save-temps:
rcx_api-hip-amdgcn-amd-amdhsa-gfx950.s) kernel by kernel: the set of kernels, each one's instruction text and its
.amdhsa_* descriptor.  The order in which the kernels were emitted may differ; local labels (.LBB<function>_<n>) are
compared without the function's number.  For a change that is meant to leave the device code alone: host-side work, or
device source that only moves.  Every kernel is put into a class:
    same    descriptor and instruction text identical
    moved   descriptor identical, the same number of basic blocks, and each basic block holds the same multiset of
            instructions once register numbers are masked (the compiler scheduled or numbered a stretch differently)
    differs anything else; the exit status is non-zero if there is one, or if the sets of kernels differ

    python tools/diag/kernel_diff.py before/rcx_api-hip-amdgcn-amd-amdhsa-gfx950.s after/rcx_api-hip-amdgcn-amd-amdhsa-gfx950.s

--rename PATTERN REPLACEMENT (may be given more than once, applied in order): a regular expression substituted in the
second file's text before anything is compared, for a change that renames kernels and is meant to do nothing else.
"""
import re
import sys


def kernels(path, renames=()):
    txt = open(path).read()
    for pattern, replacement in renames:
        txt = re.sub(pattern, replacement, txt)
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", txt, re.S):
        name = m.group(1)
        body = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)
        text = None
        if body:
            text = re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", body.group(1))
            text = "\n".join(l.split(";")[0].rstrip() for l in text.split("\n") if l.split(";")[0].strip())
        out[name] = (text, m.group(2))
    return out


def blocks(text):
    """The basic blocks of a kernel, in order: a label begins one, a branch or s_endpgm ends one.  Each as the sorted
    list of its instructions with register numbers masked (v12 -> v#, s[4:5] -> s[#], vcc / exec / m0 stay)."""
    out, cur = [], []
    for line in text.split("\n"):
        ins = re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1#", line.strip())
        if ins.endswith(":") and cur:
            out.append(sorted(cur))
            cur = []
        cur.append(ins)
        if re.match(r"s_c?branch|s_endpgm|s_setpc", ins):
            out.append(sorted(cur))
            cur = []
    return out + ([sorted(cur)] if cur else [])


def classify(a, b):
    if a[0] is None or b[0] is None or a[1] != b[1]:
        return "differs"
    if a[0] == b[0]:
        return "same"
    return "moved" if blocks(a[0]) == blocks(b[0]) else "differs"


def main():
    args, renames = sys.argv[1:], []
    while "--rename" in args:
        i = args.index("--rename")
        if i + 2 >= len(args):
            raise SystemExit("usage: kernel_diff.py BEFORE.s AFTER.s [--rename PATTERN REPLACEMENT]... [-v]")
        renames.append((args[i + 1], args[i + 2]))
        del args[i:i + 3]
    a, b = kernels(args[0]), kernels(args[1], renames)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    cls = {k: classify(a[k], b[k]) for k in sorted(set(a) & set(b))}
    moved, differ = [k for k in cls if cls[k] == "moved"], [k for k in cls if cls[k] == "differs"]
    print(f"{len(a)} kernels before, {len(b)} after; only before {len(only_a)}, only after {len(only_b)}; "
          f"same {len(cls) - len(moved) - len(differ)}, moved {len(moved)}, differs {len(differ)}")
    for what, names in (("only before", only_a), ("only after", only_b), ("moved", moved), ("differs", differ)):
        for k in names:
            print(f"  {what}: {k}")
    if "-v" in args[2:]:
        for k in cls:
            print(f"  {cls[k]:8s}{k}")
    raise SystemExit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
