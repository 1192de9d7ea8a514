"""The adaptive quad decoder's pass of 64 symbols: rcx_dec_quad_k decodes 64 symbols at a go while
every block of the wave has them, keeps the pass's four 16-byte groups in registers and stores them behind the next pass's
first top-up; the loop of 16 behind it finishes the whole groups that are left (fewer than four) and takes over the last
pass's 64 bytes, and the symbol-by-symbol tail finishes the ragged end.

What is driven here are the boundaries between the three loops: lengths with no pass, one pass and nothing else, a pass
and one or three groups, two and three passes, a pass and a tail, all three loops; a wave whose shortest block ends the
pass early for the others; waves with idle quads that decode along; items at every output alignment, whose passes store
to byte addresses; a target past the table in every group of a pass, among valid blocks; the cold refill of the input
ring in the second, third and fourth group of a pass.  The reference is the oracle: its streams, and what it decodes from
each damaged stream alone (include/rcx.h, "Damaged streams").  Every buffer is guarded (gpu_support.Guarded).
"""
import numpy as np
import pytest

from adaptive_cases import ALL_THREE, PASS_BURST_GROUPS, pass_burst_blocks
from adaptive_cases import PASS_BLOCK as BLOCK
from adaptive_cases import PASS_LENGTHS as LENGTHS  # no pass ... five passes, three groups, seven symbols one by one
from adaptive_walk import past_the_table
from cpprcoder_amd import rcx, workloads
from gpu_support import Damaged, assert_same_blocks, check_call, check_items, context, gpu_decode, gpu_encode, oracle_streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SOURCES = ("uniform", "zipf")


@pytest.fixture(scope="module")
def contexts():
    """quads16: a wave carries 16 blocks (the bench's shape); quads4: 4 blocks and 12 quads that decode along; default: for
    the few blocks of these tests one block a wave and 15 quads that decode along."""
    cs = {"quads16": context({"RCX_DEC_QUADS": "16"}), "quads4": context({"RCX_DEC_QUADS": "4"}), "default": context({})}
    yield cs
    for c in cs.values():
        c.close()


def blocks_round_trip(ctx, oracle, data, block, label):
    """The GPU's streams are the oracle's, and the GPU decodes them to the data (every buffer guarded)."""
    slots, sizes = oracle.encode_blocks(data, block, threads=4)
    payload, offsets, _ = gpu_encode(ctx, data, block)
    assert_same_blocks(payload, offsets, slots, sizes, label)
    back, st, _ = gpu_decode(ctx, payload, offsets, len(data), block)
    assert st == rcx.OK, label
    assert np.array_equal(back, data), (label, "first wrong byte", int(np.nonzero(back != data)[0][0]))
    assert ctx.last_redo(len(sizes)) == 0, label


# ---- 1. one wave of 16 blocks of one length ------------------------------------------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("length", LENGTHS)
def test_sixteen_blocks_of_one_length(contexts, oracle, length, source):
    """As blocks (a length that is no multiple of 16 leaves outputs unaligned, and that wave is decoded symbol by symbol)
    and as items (which keep the fast loops at any alignment)."""
    data = workloads.by_name(source, 16 * length, 8000 + length)
    blocks_round_trip(contexts["quads16"], oracle, data, length, (length, source, "blocks"))
    items = [data[k * length: (k + 1) * length] for k in range(16)]
    check_items(contexts["quads16"], items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE), label=(length, source, "items"))


# ---- 2. mixed lengths: the pass ends where the wave's shortest block has no 64 symbols left --------------------------------
@pytest.mark.parametrize("where", [0, 15], ids=["first_quad", "last_quad"])
@pytest.mark.parametrize("short", [BLOCK - 16, BLOCK - 64, 65])
def test_one_short_block_in_the_wave(contexts, oracle, short, where):
    lengths = [BLOCK] * 16
    lengths[where] = short
    data = workloads.by_name("zipf", sum(lengths), 8100 + short)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    items = [data[bounds[k]: bounds[k + 1]] for k in range(16)]
    check_items(contexts["quads16"], items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE), label=(short, where, "items"))
    if where == 15 and short % 16 == 0:  # the block geometry's short block is its last one
        blocks_round_trip(contexts["quads16"], oracle, data, BLOCK, (short, "blocks"))


@pytest.mark.parametrize("name", ["default", "quads4"])
@pytest.mark.parametrize("count", [1, 4])
def test_idle_quads_decode_along(contexts, oracle, count, name):
    """Fewer blocks than quads: the wave's other quads decode a block along and store nothing."""
    lengths = [ALL_THREE, BLOCK, 129, 192][:count]
    data = workloads.by_name("zipf", sum(lengths), 8200 + count)
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    items = [data[bounds[k]: bounds[k + 1]] for k in range(count)]
    check_items(contexts[name], items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE), label=(count, name, "items"))
    whole = workloads.by_name("uniform", (count - 1) * BLOCK + ALL_THREE, 8300 + count)  # aligned blocks, the last one ragged
    blocks_round_trip(contexts[name], oracle, whole, BLOCK, (count, name, "blocks"))


# ---- 3. items whose outputs begin at every alignment ---------------------------------------------------------------------
@pytest.mark.parametrize("base", [64, 192])
def test_items_at_every_alignment(contexts, oracle, base):
    """Sizes base + 0 .. base + 15 and one more: the 17 outputs begin at all 16 residues mod 16.  base 64: one pass, its
    bytes leave behind the loops; base 192: three passes, two of which store theirs behind the next one's top-up."""
    lengths = [base + r for r in range(16)] + [base]
    bounds = np.concatenate([[0], np.cumsum(lengths)])
    assert {int(b) % 16 for b in bounds[:-1]} == set(range(16))
    data = workloads.by_name("zipf", int(bounds[-1]), 8400 + base)
    items = [data[bounds[k]: bounds[k + 1]] for k in range(len(lengths))]
    want = oracle_streams(oracle, items, rcx.CODER_ADAPTIVE)
    for name in ("quads16", "default"):
        for out_offset in (0, 5):
            check_items(contexts[name], items, want, out_offset=out_offset, label=(base, name, out_offset))


# ---- 4. a target past the table in a pass --------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [0, 1, 2, 3])
@pytest.mark.parametrize("which", ["first_pass", "late_pass"])
def test_target_past_the_table_in_a_pass(contexts, oracle, which, group):
    """At in-group positions 0, 1 and 15 of one of the pass's four groups, in one block among 15 valid ones of the same
    wave: the block is marked and decoded again, every block's bytes are what the oracle gives for its stream alone, and
    nothing outside the output is written.  In a pass the scratch row, which such a block reads as counts, holds no
    output."""
    groups = [group] if which == "first_pass" else [4 * p + group for p in range(20, 40)]
    for position in (0, 1, 15):
        seed = 8500 + 16 * group + position
        data = workloads.by_name("zipf", 16 * BLOCK, seed)
        d = Damaged(oracle, data, BLOCK, rcx.CODER_ADAPTIVE, seed)
        made = None
        # in another quad for every group and position (whether a symbol leaves room behind the table depends on the data)
        for b in ((5 * group + 3 * position + k) % 16 for k in range(16)):
            made = past_the_table(d, b, position, groups=groups)
            if made is not None:
                break
        if which == "first_pass" and group == 0 and position == 0:
            # the first symbol's range, 2^32 - 256, is a multiple of its total, 256: no target lies past the table there
            assert made is None
            continue
        assert made is not None, (which, group, position)
        stream, at_symbol = made
        assert at_symbol % 16 == position and (at_symbol // 16) % 4 == group and (at_symbol < 64) == (which == "first_pass")
        d.damage(b, f"target past the table at symbol {at_symbol}", stream)
        ok, out = d.decode_one(b)
        assert ok and np.array_equal(out[:at_symbol], d.good(b)[:at_symbol]) and out[at_symbol] == 0
        for name in ("quads16", "default"):
            check_call(contexts[name], d, BLOCK, 0, (name, which, group, position))
            assert contexts[name].last_redo(16) == 1, (name, which, group, position)


# ---- 5. the cold refill in the second, third and fourth group of a pass -----------------------------------------------------
@pytest.mark.parametrize("group", PASS_BURST_GROUPS)
def test_cold_refill_inside_a_pass(contexts, oracle, group):
    """test_bursts_of_very_improbable_symbols at 4 KiB blocks: after some 3000 equal bytes every other value costs about 12
    bits, 6 dwords per 16 symbols where the top-up supplies 4, so the input ring runs low and the synchronous refill runs,
    again and again every few groups for the 32 groups the burst lasts.  The burst begins two groups in front of
    group `group` of a pass, in a pass of its own in every other block, and all 16 blocks of a wave share the top-up's
    branch: the refill is taken in front of every group of a pass."""
    data = np.concatenate(pass_burst_blocks(group))  # (the builder: tests/adaptive_cases.py)
    for name in ("quads16", "default"):
        blocks_round_trip(contexts[name], oracle, data, BLOCK, (name, group))
