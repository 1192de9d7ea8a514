#!/usr/bin/env python3
"""Static instruction counts of a kernel's largest basic block (for rcx_dec_quad_k: a group of 16 symbols of the pass of
64; before it, the loop of 16), the figures DESIGN 3.4 quotes per round.  Input is the device assembly of

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S cpprcoder_amd/csrc/rcx_api.hip -o rcx_api.s
    python tools/diag/count_block.py rcx_api.s [KERNEL_REGEX]      (default: rcx_dec_quad_k<4, RcxBlocks>)

The rule: the kernel's text from its label to .Lfunc_end; comments (from ';') and directives (lines starting with '.')
dropped; a label ends a block, and so does a branch (s_branch, s_cbranch_*, s_setpc, s_endpgm), which still belongs to
the block it ends.  Of the longest block: vector = mnemonics starting with v_, ds = ds_, and s_nop and s_waitcnt by name.
The inline-assembly sequences count like everything else.  Take the counts again after any change of toolchain: where the
compiler puts its s_nop depends on its register allocation.

The second line divides by the symbols in the block, one ds_read_b128 (the leaf read) each.  The top-up's cold branch
ends a block, so the pass of 64 symbols is four blocks and what lies between them; the third part of the output is
therefore the loop around the longest block -- from the target of the first backward branch behind it to that branch --
block by block, with the same counts, scalar instructions (s_ but s_nop and s_waitcnt), branches, global stores and the
16-byte LDS writes and reads.  A loop inside that loop, with the jump into it, is the top-up's synchronous refill and is
marked `cold`; the other blocks are what a pass goes through on ordinary data and add up to it.
"""
import re
import sys

BRANCH = r"s_c?branch|s_endpgm|s_setpc"
COLUMNS = (("instructions", r""), ("vector", r"v_"), ("ds", r"ds_"), ("s_nop", r"s_nop"), ("s_waitcnt", r"s_waitcnt"),
           ("scalar", r"s_(?!nop|waitcnt)"), ("branches", BRANCH), ("global stores", r"global_store|flat_store"),
           ("ds_write_b128", r"ds_write_b128"), ("ds_read_b128", r"ds_read_b128"))


def basic_blocks(txt, pattern):
    """-> (kernel name, [(label or None, [instructions])]) in the order of the text"""
    m = re.search(r"^(" + pattern + r"\S*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M)
    if not m:
        raise SystemExit(f"no kernel matches {pattern}")
    blocks, cur, label = [], [], None
    for line in m.group(2).split("\n"):
        ins = line.split(";")[0].strip()
        if not ins:
            continue
        if ins.endswith(":"):
            blocks.append((label, cur))
            cur, label = [], ins[:-1]
            continue
        if ins.startswith("."):
            continue
        cur.append(ins)
        if re.match(BRANCH, ins):
            blocks.append((label, cur))
            cur, label = [], None
    blocks.append((label, cur))
    return m.group(1), blocks


def largest_block(txt, pattern):
    name, blocks = basic_blocks(txt, pattern)
    return name, max((b for _, b in blocks), key=len)


def count(block, p):
    return sum(1 for i in block if re.match(p, i))


def loop_around(blocks, at):
    """The blocks from the target of the first backward branch behind block `at` that reaches back to it or past it, to
    that branch; None if there is none."""
    where = {label: k for k, (label, _) in enumerate(blocks) if label}
    for k in range(at, len(blocks)):
        ins = blocks[k][1]
        if ins and re.match(r"s_c?branch", ins[-1]):
            target = where.get(ins[-1].split()[-1])
            if target is not None and target <= at:
                return target, k
    return None


def main():
    pattern = sys.argv[2] if len(sys.argv) > 2 else r"_Z14rcx_dec_quad_kILi4E9RcxBlocksE"
    name, blocks = basic_blocks(open(sys.argv[1]).read(), pattern)
    at = max(range(len(blocks)), key=lambda k: len(blocks[k][1]))
    block = blocks[at][1]
    print(name)
    print(f"instructions {len(block)}  vector {count(block, r'v_')}  ds {count(block, r'ds_')}  s_nop {count(block, r's_nop')}  s_waitcnt {count(block, r's_waitcnt')}  "
          f"64-bit multiply-adds {count(block, r'v_mad_[iu]64')}  v_cndmask {count(block, r'v_cndmask')}  v_mov {count(block, r'v_mov')}")
    symbols = count(block, r"ds_read_b128")
    if symbols:
        print(f"per symbol ({symbols} in the block): " + "  ".join(f"{what} {count(block, p) / symbols:.2f}" for what, p in COLUMNS[:6]))
    span = loop_around(blocks, at)
    if span:
        first, last = span
        where = {label: k for k, (label, _) in enumerate(blocks) if label}
        print(f"the loop around it, {blocks[first][0]} to the branch that closes it:")
        print("  " + " ".join(f"{what:>13s}" for what, _ in COLUMNS) + "  block")
        cold_blocks = set()
        for k in range(first, last):
            ins = blocks[k][1]
            target = where.get(ins[-1].split()[-1]) if ins and re.match(r"s_c?branch", ins[-1]) else None
            if target is not None and first < target <= k:  # a loop inside the loop, and the jump into it
                cold_blocks.update(range(target, k + 1))
                before = next((j for j in range(target - 1, first, -1) if blocks[j][1]), None)
                if before is not None and blocks[before][1][-1].startswith("s_branch"):
                    cold_blocks.add(before)
        for k in range(first, last + 1):
            label, ins = blocks[k]
            if not ins:
                continue
            cold = " cold" if k in cold_blocks else ""
            print("  " + " ".join(f"{count(ins, p):13d}" for _, p in COLUMNS) + f"  {label or '':12s} {ins[-1] if re.match(BRANCH, ins[-1]) else ''}{cold}")


if __name__ == "__main__":
    main()
