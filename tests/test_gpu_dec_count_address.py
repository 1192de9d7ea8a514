"""The adaptive quad decoder's count address as one bit insert: a symbol is carried to the next one
scaled by 4 -- 4 x symbol = (the lane's three borrows << 2) + 64 x node + 4 x the lane's last symbol --, the address of its
count is v_bfi_b32 pad, 12, psym4, pla (bits 2 and 3 of the scaled symbol into the 16-byte aligned address of the lane's
four counts), and its byte is (psym4 & owner) shifted into the output word at PSHIFT - 2, or down by 2 for a word's first
byte.  The last symbol of a group and every symbol of the tail go through RCX_QUAD_DEC_FINISH, which does the same.

What is driven here: every count slot 0 .. 3 of every lane as the decoded symbol at every in-group position, in the pass
of 64, the loop of 16 and the symbol-by-symbol tail (so the four positions that begin an output word and the closing one
see all four slots); a block with idle quads that decode along; a target past the table, whose borrows are arbitrary
words, at the positions where the address is formed differently (first of a group, behind it, a word's first byte, the
closing symbol).  The reference is the oracle: its streams, and what it decodes from each damaged stream alone.  Every
buffer is guarded (gpu_support.Guarded).  The last test needs no GPU: the bit insert and the scaled byte as integer
arithmetic, in the style of test_quad_round2_words.py.
"""
import numpy as np
import pytest

from adaptive_cases import PASS_BLOCK as BLOCK
from adaptive_walk import past_the_table
from cpprcoder_amd import rcx, workloads
from gpu_support import Damaged, assert_same_blocks, check_call, check_items, context, gpu_decode, gpu_encode, oracle_streams

torch = pytest.importorskip("torch")

SOURCES = ("uniform", "zipf")
LENGTHS = (64 + 16 + 7, 256)  # a pass, a group and seven symbols one by one; four passes
M = 0xFFFFFFFF


@pytest.fixture(scope="module")
def contexts():
    cs = {"quads16": context({"RCX_DEC_QUADS": "16"}), "default": context({})}
    yield cs
    for c in cs.values():
        c.close()


def cycling_blocks(source, length, nblocks, seed):
    """`nblocks` blocks of `length` bytes of the workload `source` whose low four bits -- the lane j and its slot s of the
    byte's count, 4j + s -- are replaced by (index in the block + block number) mod 16: block b cycles through the values
    16n + 4j + s with the workload's nodes n, and the 16 blocks of a wave put every (j, s) at every in-group position."""
    data = workloads.by_name(source, nblocks * length, seed).reshape(nblocks, length)
    i, b = np.arange(length)[None, :], np.arange(nblocks)[:, None]
    return ((data & 0xF0) | ((i + b) & 15)).astype(np.uint8)


def loop_of(i, length, fast):
    """Which loop decodes symbol i of a block of `length` bytes whose wave runs the fast loops (`fast`): 0 the pass of 64,
    1 the loop of 16, 2 symbol by symbol."""
    if not fast:
        return 2
    return 0 if i < (length & ~63) else 1 if i < (length & ~15) else 2


def assert_every_slot_everywhere(blocks, fast):
    """Every lane j and slot s is the decoded symbol at every in-group position of every loop the blocks run through."""
    nblocks, length = blocks.shape
    seen = set()
    for b in range(nblocks):
        for i in range(length):
            v = int(blocks[b, i])
            seen.add((loop_of(i, length, fast), i % 16, (v >> 2) & 3, v & 3))
    for loop in {loop_of(i, length, fast) for i in range(length)}:
        positions = {i % 16 for i in range(length) if loop_of(i, length, fast) == loop}
        assert positions == set(range(16)) or loop == 2, (loop, positions)
        for p in positions:
            for j in range(4):
                for s in range(4):
                    assert (loop, p, j, s) in seen, (loop, p, j, s)
    if fast and length >= 16:  # the four positions whose byte begins an output word, and the closing symbol of a group
        assert all((lp, p, j, s) in seen for lp in {loop_of(0, length, fast)} for p in (3, 7, 11, 15) for j in range(4) for s in range(4))


# ---- 1. sixteen blocks in one wave, every slot used ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("length", LENGTHS)
def test_every_slot_at_every_position(contexts, oracle, length, source):
    """As blocks (a length that is no multiple of 16 leaves outputs unaligned: that wave is decoded symbol by symbol, every
    byte and count by RCX_QUAD_DEC_FINISH) and as items (which keep the fast loops at any alignment)."""
    blocks = cycling_blocks(source, length, 16, 9000 + length)
    aligned = length % 16 == 0
    assert_every_slot_everywhere(blocks, fast=aligned)  # as blocks
    assert_every_slot_everywhere(blocks, fast=True)     # as items
    ctx, data = contexts["quads16"], blocks.reshape(-1)
    slots, sizes = oracle.encode_blocks(data, length, threads=4)
    payload, offsets, _ = gpu_encode(ctx, data, length)
    assert_same_blocks(payload, offsets, slots, sizes, (length, source, "blocks"))
    back, st, _ = gpu_decode(ctx, payload, offsets, len(data), length)
    assert st == rcx.OK, (length, source)
    assert np.array_equal(back, data), (length, source, "first wrong byte", int(np.nonzero(back != data)[0][0]))
    assert ctx.last_redo(16) == 0, (length, source)
    items = [blocks[k] for k in range(16)]
    check_items(ctx, items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE), label=(length, source, "items"))


# ---- 2. one block with idle quads ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("source", SOURCES)
def test_one_item_with_idle_quads(contexts, oracle, source):
    """A 129-byte item in the default context: one quad carries it, the wave's other fifteen decode it along -- the same
    bit inserts into their own tables -- and store nothing.  Two passes and a symbol by itself."""
    items = [cycling_blocks(source, 129, 1, 9100)[0]]
    assert {int(v) & 15 for v in items[0]} == set(range(16))
    check_items(contexts["default"], items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE), label=(source, "one item"))


# ---- 3. a target past the table among fifteen valid blocks ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("position", [0, 1, 3, 15])
@pytest.mark.parametrize("which", ["first_pass", "late_pass"])
def test_target_past_the_table(contexts, oracle, which, position):
    """Round 1 then takes "node 16", the scratch row is read as counts and the three borrows, so the scaled symbol, are
    arbitrary words: the bit insert keeps the ds_add inside the lane's 16 bytes of that row.  Positions: 0 (the count of
    the symbol before it is made by the closing sequence of the group before), 1 (the first made by a next symbol), 3
    (its byte begins an output word), 15 (made by RCX_QUAD_DEC_FINISH).  In a late pass the row holds skipped ring
    pieces, i.e. stream bytes.  The block is marked and decoded again; every block's bytes are what the oracle gives for
    its stream alone; the guards are intact (gpu_decode)."""
    groups = range(0, 4) if which == "first_pass" else range(80, 160)
    seed = 9200 + position + (100 if which == "late_pass" else 0)
    data = workloads.by_name("zipf", 16 * BLOCK, seed)
    d = Damaged(oracle, data, BLOCK, rcx.CODER_ADAPTIVE, seed)
    made = None
    for b in ((3 * position + k) % 16 for k in range(16)):
        made = past_the_table(d, b, position, groups=groups)
        if made is not None:
            break
    assert made is not None, (which, position)
    stream, at_symbol = made
    assert at_symbol % 16 == position and (at_symbol < 64) == (which == "first_pass")
    d.damage(b, f"target past the table at symbol {at_symbol}", stream)
    ok, out = d.decode_one(b)
    assert ok and np.array_equal(out[:at_symbol], d.good(b)[:at_symbol]) and out[at_symbol] == 0
    for name in ("quads16", "default"):
        check_call(contexts[name], d, BLOCK, 0, (name, which, position))
        assert contexts[name].last_redo(16) == 1, (name, which, position)


# ---- 4. the arithmetic, on the host ------------------------------------------------------------------------------------------
def bfi(mask, a, b):
    """v_bfi_b32: the bits of a where mask is set, those of b elsewhere"""
    return (mask & a) | (~mask & b & M)


def test_bit_insert_and_scaled_byte_as_integers():
    rs = np.random.RandomState(23)
    n = 50000
    # (a) arbitrary 32-bit psym4, any 16-byte aligned pla: the address stays within [pla, pla + 12], dword aligned
    psym4 = rs.randint(0, 1 << 32, n, dtype=np.int64)
    psym4[:6] = (0, M, 12, M - 12, 1 << 31, 3)
    pla = rs.randint(0, 1 << 28, n, dtype=np.int64) << 4
    pla[:3] = (0, M & ~15, 16)
    pad = bfi(12, psym4, pla)
    assert ((pad >= pla) & (pad <= pla + 12) & (pad % 4 == 0)).all()
    assert set(np.unique(pad - pla)) == {0, 4, 8, 12}
    # the kernel's pla: the lane's 16 bytes of row `node` (0 .. 16) of the block's quarter of its table group
    GROUP_BYTES, ROW, QUARTER = 4352, 256, 64
    group, quarter, lane, node = rs.randint(0, 4, n), rs.randint(0, 4, n), rs.randint(0, 4, n), rs.randint(0, 17, n)
    row = group * GROUP_BYTES + quarter * QUARTER + ROW * node
    pla = row + 16 * lane
    assert (pla % 16 == 0).all()
    pad = bfi(12, psym4, pla)
    assert ((pad >= pla) & (pad + 4 <= pla + 16) & (pad + 4 <= row + QUARTER) & (pad + 4 <= (group + 1) * GROUP_BYTES)).all()
    # the form that is NOT used, pla + 4 x the borrows + 12, leaves the lane's 16 bytes on arbitrary borrows
    hs = rs.randint(0, 1 << 32, n, dtype=np.int64)
    stray = (pla + 4 * hs + 12) & M
    assert ((stray < pla) | (stray > pla + 12)).any()
    # (b) valid high words -- three borrows, 0 or -1 each, in the owning lane -- : today's symbol, address and byte
    node = rs.randint(0, 16, n).astype(np.int64)
    h = -rs.randint(0, 2, (n, 3)).astype(np.int64)
    h[:8] = [[-(k >> 2 & 1), -(k >> 1 & 1), -(k & 1)] for k in range(8)]
    own = np.where(rs.randint(0, 2, n) == 1, M, 0).astype(np.int64)
    own[:8] = M
    sym = (node * 16 + 4 * lane + 3 + h.sum(axis=1)) & M                 # v_add3_u32 sym, sb, ha, hb; v_add_u32 sym, sym, hc
    pad_old = (((sym & 3) << 2) + pla) & M                               # v_and_b32 pad, 3, psym; v_lshl_add_u32 pad, pad, 2, pla
    hs = h.sum(axis=1) & M                                               # v_add3_u32 hs, ha, hb, hc
    sb4 = (node << 6) | (4 * (4 * lane + 3))                             # v_lshl_or_b32 sb4, node, 6, 4 x (4j + 3)
    assert (sb4 == (node << 6) + 16 * lane + 12).all()
    sym4 = ((hs << 2) + sb4) & M                                         # v_lshl_add_u32 psym4, phs, 2, psb4
    assert (sym4 == 4 * sym).all() and (sym < 256).all()
    assert (bfi(12, sym4, pla) == pad_old).all()
    assert {(int(a), int(b)) for a, b in zip(lane, sym & 3)} == {(j, s) for j in range(4) for s in range(4)}
    byte = sym & own
    word = rs.randint(0, 1 << 32, n, dtype=np.int64)
    got0 = (sym4 & own) >> 2                                             # v_and_b32 pword, psym4, pown; v_lshrrev_b32 pword, 2, pword
    assert (got0 == byte).all()                                          # PSHIFT 0: the byte is the word
    for pshift in (8, 16, 24):
        below = word & ((1 << pshift) - 1)                               # the bytes made so far lie below PSHIFT
        got = (((sym4 & own) << (pshift - 2)) & M) | below               # v_and_b32 pye, psym4, pown; v_lshl_or_b32 pword, pye, PSHIFT - 2, pword
        assert (got == ((byte << pshift) | below)).all(), pshift
    assert (byte[own == M] == sym[own == M]).all() and (byte[own == 0] == 0).all()
