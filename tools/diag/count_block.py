#!/usr/bin/env python3
"""Static instruction counts of a kernel's largest basic block (for rcx_dec_quad_k: the fast loop's 16 symbols), the
figures DESIGN 3.4 quotes per round.  Input is the device assembly of

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S cpprcoder_amd/csrc/rcx_api.hip -o rcx_api.s
    python tools/diag/count_block.py rcx_api.s [KERNEL_REGEX]      (default: rcx_dec_quad_k<4, RcxBlocks>)

The rule: the kernel's text from its label to .Lfunc_end; comments (from ';') and directives (lines starting with '.')
dropped; a label ends a block, and so does a branch (s_branch, s_cbranch_*, s_setpc, s_endpgm), which still belongs to
the block it ends.  Of the longest block: vector = mnemonics starting with v_, ds = ds_, and s_nop and s_waitcnt by name.
The inline-assembly sequences count like everything else.  Take the counts again after any change of toolchain: where the
compiler puts its s_nop depends on its register allocation.
"""
import re
import sys


def largest_block(txt, pattern):
    m = re.search(r"^(" + pattern + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)
    if not m:
        raise SystemExit(f"no kernel matches {pattern}")
    blocks, cur = [], []
    for line in m.group(2).split("\n"):
        ins = line.split(";")[0].strip()
        if not ins:
            continue
        if ins.endswith(":"):
            blocks.append(cur)
            cur = []
            continue
        if ins.startswith("."):
            continue
        cur.append(ins)
        if re.match(r"s_c?branch|s_endpgm|s_setpc", ins):
            blocks.append(cur)
            cur = []
    blocks.append(cur)
    return m.group(1), max(blocks, key=len)


def main():
    pattern = sys.argv[2] if len(sys.argv) > 2 else r"_Z14rcx_dec_quad_kILi4E9RcxBlocksE"
    name, block = largest_block(open(sys.argv[1]).read(), pattern)
    count = lambda p: sum(1 for i in block if re.match(p, i))
    print(name)
    print(f"instructions {len(block)}  vector {count(r'v_')}  ds {count(r'ds_')}  s_nop {count(r's_nop')}  s_waitcnt {count(r's_waitcnt')}  "
          f"64-bit multiply-adds {count(r'v_mad_[iu]64')}  v_cndmask {count(r'v_cndmask')}  v_mov {count(r'v_mov')}")


if __name__ == "__main__":
    main()
