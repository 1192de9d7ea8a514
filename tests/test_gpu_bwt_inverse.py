"""The inverse block sort (csrc/rcx_bwt.hpp, rcx_bwt_inv_k; blksort.h:543-679) at the points where it changes path: the
blocks of tests/bwt_inverse_cases.py, whose pieces, marks, links and cycles, and whose batches on either side of the
counting pass's pile switch, tests/test_bwt_inverse_cases_cpu.py asserts.  Every expected byte is the oracle's inverse
of the same block (the oracle restates blksort.h and is pinned to the reference build on these blocks too,
tests/test_oracle_bwt.py); the model only aims the inputs and deals them out.

Every test runs in both forms of the counting pass's rank, as gpu_support.bwt_ctx makes the contexts: with ballots and
with RCX_BWT_MATCH=atomic.  Under the latter the library takes the atomic form only if its check of the device's LDS
lane order holds, and nothing reports which form ran: on a device where the check failed both runs would be the ballot
form."""
import numpy as np
import pytest

import bwt_inverse_cases as ic
import oracle_lib
from bwt_cases import BLOCK, ENCODED
from gpu_support import Guarded
from gpu_support import bwt_ctx as ctx  # noqa: F401  (both rank forms)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FAMILIES = ("descent", "rotation", "steps3", "modulo", "exact_32", "pile")


@pytest.fixture(scope="module")
def cases():
    """family -> [(name, block, the oracle's inverse of it)], made once for both rank forms and never written to."""
    o = oracle_lib.oracle()
    out = {}
    for family, items in ic.all_cases().items():
        want = o.bwt_decode(np.concatenate([blk for _, blk in items]), threads=16)
        out[family] = [(name, blk, want[i * BLOCK:(i + 1) * BLOCK]) for i, (name, blk) in enumerate(items)]
    assert tuple(out) == FAMILIES
    return out


@pytest.fixture(scope="module")
def rings(cases):
    """The blocks by what their walk leaves in LDS, by the model: [with marks, the most first], [no marks, a cycle of 32
    rows or more], [no marks, a cycle below 32]."""
    out = [[], [], []]
    for family in FAMILIES:
        for item in cases[family]:
            walk = ic.inverse_walk(*ic.split(item[1]))
            out[0 if walk.marks else 2 if walk.cycle < 32 else 1].append((-walk.marks, item))
    return [[item for _, item in sorted(ring, key=lambda x: x[0])] for ring in out]


def same_blocks(got, items, what):
    """`got`: the decoded bytes of `items` (name, block, expected) in their order; every block that differs is named."""
    assert len(got) == BLOCK * len(items), (what, len(got))
    bad = []
    for i, (name, _, want) in enumerate(items):
        mine = got[i * BLOCK:(i + 1) * BLOCK]
        if not np.array_equal(mine, want):
            at = int(np.nonzero(mine != want)[0][0])
            bad.append(f"block {i}, {name}: {int(np.count_nonzero(mine != want))} bytes differ, the first at {at} "
                       f"(got {int(mine[at])}, want {int(want[at])})")
    assert not bad, f"{what}: {len(bad)} of {len(items)} blocks differ from the oracle's inverse\n" + "\n".join(bad[:40])


@pytest.mark.parametrize("family", FAMILIES)
def test_a_family_is_the_oracles_inverse(ctx, cases, family):
    """descent: one cycle of 1 ... 254 rows among fixed points (1, 2, 3 and 8 pieces on the walk, the first piece running
    into itself, first and residue at 0 and at 1023 and 31).  rotation: cycles that do not divide 32768, 32 ... 1024 pieces
    on the walk with 512, 513 and 514 among them (the tenth round of jumping is needed from 514), pieces of 31, 32 and 33
    rows, one of 31 744.  steps3: the 992 marks there can be at most (one piece of 31 745 rows), exactly two laps, marks
    off the walk.  modulo: hundreds of marks off the walk, all of them where the row is a fixed point, and four blocks
    where stretches off the walk would land inside the output if job 1 took them.  exact_32: break
    and mark on the same step in every piece.  pile: the counting pass with 32, 33 and 64 lanes of a sampled batch on one
    digit, even and odd, both halves of a count's dword, waves on different sides, the histogram's extremes."""
    items = cases[family]
    got = ctx.bwt_decode(np.concatenate([blk for _, blk, _ in items]))
    same_blocks(got, items, family)


def test_all_families_in_one_call(ctx, rings):
    """At least three blocks per compute unit in one call (a workgroup per CU takes blocks off a counter), dealt so that
    blocks with marks -- the most first --, blocks with none and blocks with a cycle below 32 follow each other, along the
    call and from a block to the one a device's width further on: a workgroup's LDS (misc[40], mark_of, lens, link) goes
    from each kind to each other.  That is arranged, not asserted: which workgroup takes which block cannot be seen."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert all(rings)
    total = 3 * max(cus, *(len(r) for r in rings))
    taken, items = [0, 0, 0], []
    for i in range(total):
        kind = (i + i // cus) % 3
        items.append(rings[kind][taken[kind] % len(rings[kind])])
        taken[kind] += 1
    assert all(taken[k] >= len(rings[k]) for k in range(3))          # every block is in the call
    got = ctx.bwt_decode(np.concatenate([blk for _, blk, _ in items] + [np.arange(77, dtype=np.uint8)]))
    assert np.array_equal(got[BLOCK * len(items):], np.arange(77, dtype=np.uint8))   # the tail behind the blocks is copied
    same_blocks(got[: BLOCK * len(items)], items, f"{len(items)} blocks on {cus} compute units")


@pytest.mark.parametrize("shift,oshift", ((1, 3), (7, 9), (15, 15)))
def test_device_call_off_its_16_byte_borders(ctx, cases, shift, oshift):
    """The longest piece, the shortest cycles and the pile blocks through rcx_bwt_decode_device, the source `shift` bytes
    behind a 16-byte border and the destination `oshift` behind one: the block's image in LDS and the staged output are
    shifted (`shift`, `oshift` in the kernel).  The source and the bytes around the output stay as they were."""
    by_name = {item[0]: item for family in FAMILIES for item in cases[family]}
    items = [by_name["steps3(a=1, b=31)"], by_name["descent(C=1, lead=0)"], by_name["rotation(M=32767, s=32, lead=0)"],
             by_name["descent(C=2, lead=17)"], by_name["steps3(a=16383, b=2)"]] + cases["pile"]
    enc = np.concatenate([blk for _, blk, _ in items])
    src = Guarded(len(enc), shift, enc, salt=1)
    dst = Guarded(BLOCK * len(items), oshift, salt=2)
    assert src.view.data_ptr() % 16 == shift and dst.view.data_ptr() % 16 == oshift
    ctx.bwt_decode_device(src.view, len(enc), dst.view)
    ctx.sync_status()
    src.check(0, "decode src")
    dst.check(BLOCK * len(items), "decode dst")
    same_blocks(dst.view.cpu().numpy(), items, f"shift {shift}, oshift {oshift}")
    assert len(enc) == ENCODED * len(items)
