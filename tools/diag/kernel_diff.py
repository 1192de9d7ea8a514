#!/usr/bin/env python3
"""Is the device code of two builds the same?  Compares two gfx950 assembly files (hipcc --save-temps:
rcx_api-hip-amdgcn-amd-amdhsa-gfx950.s) kernel by kernel: the set of kernels, each one's instruction text and its
.amdhsa_* descriptor.  The order in which the kernels were emitted may differ; local labels (.LBB<function>_<n>) are
compared without the function's number.  For a change that is meant to touch the host side only.

    python tools/diag/kernel_diff.py before/rcx_api-hip-amdgcn-amd-amdhsa-gfx950.s after/rcx_api-hip-amdgcn-amd-amdhsa-gfx950.s
"""
import re
import sys


def kernels(path):
    txt = open(path).read()
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


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [k for k in sorted(set(a) & set(b)) if a[k] != b[k] or a[k][0] is None]
    print(f"{len(a)} kernels before, {len(b)} after; only before {len(only_a)}, only after {len(only_b)}, "
          f"instruction text or descriptor differs {len(differ)}")
    for what, names in (("only before", only_a), ("only after", only_b), ("differs", differ)):
        for k in names:
            print(f"  {what}: {k}")
    raise SystemExit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
