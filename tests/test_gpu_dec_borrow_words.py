"""The adaptive quad decoder where its bounds borrow: rcx_dec_quad_k takes the borrow of low - U * t from the high word of
a 64-bit multiply-add, per bound, and raises its negated bounds by those words.

Round trips on inputs that sit on every borrow boundary -- the first and last lane of a quad, the first and last node, a
count that grows to the block's length while t shrinks -- and damaged streams whose target lies past the table at the
in-group positions where the kernel's paths part, continued with runs of 0xFF and of 0x00 (the extremes for the low and
range a block computes on after that).  The reference is the oracle: its streams, and what it decodes from each damaged
stream alone (the rule in include/rcx.h, "Damaged streams").
"""
import numpy as np
import pytest

from adaptive_cases import ONE_VALUE_BYTES, ONE_VALUE_N, one_value_block
from cpprcoder_amd import rcx, workloads
from gpu_support import Damaged, assert_same_blocks, check_call, context, gpu_decode, gpu_encode

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BLOCK = 4096
RAGGED = 1237  # the last block: 77 groups of 16 and 5 symbols one by one
REPEATED = (0, 15, 16, 63, 64, 191, 192, 255)  # first / last symbol of a node, of a lane, of the alphabet
PAIRS = ((15, 16), (63, 64), (191, 192), (0, 255))  # across a node boundary, a lane boundary (twice), both ends
DRAWN = ("zipf", "uniform", "runs")


@pytest.fixture(scope="module")
def contexts():
    cs = {"default": context({}), "quads16": context({"RCX_DEC_QUADS": "16"})}
    yield cs
    for c in cs.values():
        c.close()


def block_of(kind, n, seed):
    if kind < len(REPEATED):
        return np.full(n, REPEATED[kind], np.uint8)
    kind -= len(REPEATED)
    if kind < len(PAIRS):
        return np.array(PAIRS[kind], np.uint8)[np.random.RandomState(seed).randint(0, 2, n)]
    return workloads.by_name(DRAWN[kind - len(PAIRS)], n, seed)


KINDS = len(REPEATED) + len(PAIRS) + len(DRAWN)  # 15: every call below carries each of them at least once


def buffer_of(nblocks, first_kind):
    """nblocks blocks of BLOCK bytes and a ragged one, block b of kind (first_kind + b) mod KINDS."""
    parts = [block_of((first_kind + b) % KINDS, BLOCK if b < nblocks else RAGGED, 300 + b) for b in range(nblocks + 1)]
    return np.concatenate(parts)


@pytest.mark.parametrize("first_kind", [0, 7])  # (7: the ragged block and every place in the wave get another kind)
@pytest.mark.parametrize("nblocks", [16, 17])
def test_round_trips_on_the_borrow_boundaries(contexts, oracle, nblocks, first_kind):
    data = buffer_of(nblocks, first_kind)
    slots, sizes = oracle.encode_blocks(data, BLOCK, threads=8)
    for name, ctx in contexts.items():
        payload, offsets, _ = gpu_encode(ctx, data, BLOCK)
        assert_same_blocks(payload, offsets, slots, sizes)
        back, st, _ = gpu_decode(ctx, payload, offsets, len(data), BLOCK)
        assert st == rcx.OK, name
        assert np.array_equal(back, data), (name, int(np.nonzero(back != data)[0][0]) // BLOCK)


@pytest.mark.parametrize("byte", ONE_VALUE_BYTES)
def test_one_large_block_of_one_byte(contexts, oracle, byte):
    """2^18 symbols of one value: its count -- and every bound above it -- grows to 2^18 while t falls to range / 2^18."""
    n = ONE_VALUE_N
    data = one_value_block(byte, n)
    slots, sizes = oracle.encode_blocks(data, n)
    for name, ctx in contexts.items():
        payload, offsets, _ = gpu_encode(ctx, data, n)
        assert_same_blocks(payload, offsets, slots, sizes)
        back, st, _ = gpu_decode(ctx, payload, offsets, n, n)
        assert st == rcx.OK and np.array_equal(back, data), name


# ---------------------------------------------------------------------------------------------------------------------
# Damaged streams.  A target past the table cannot be had by flipping payload bytes at random: low stays below range on
# any input, and only the last (range mod total) values below range are past the table.  So the stream is made: the
# coder's interval along the block's first i symbols is walked in exact integers (range depends on the symbols alone; the
# decoder's low is the stream's bytes so far, as one big-endian number, minus the interval's lower end), and the bytes
# the decoder has consumed when it looks for symbol i are set to the number that puts low into those last values.
# ---------------------------------------------------------------------------------------------------------------------
def walk(symbols, steps):
    """The decoder's state in front of symbol i, for i = 0 .. steps: (i, lower end, range, t, total, bytes consumed
    counted from byte 4 of the stream).  include/rcx.h: every count starts at 1; range starts at 2^24 - 1 behind the
    four bytes of low; range is shifted up by whole bytes until its top byte is not 0, then t = range / total."""
    counts = np.ones(256, np.int64)
    total, rng, lower, nbytes = 256, 0x00FFFFFF, 0, 4
    for i in range(steps + 1):
        k = (32 - rng.bit_length()) // 8
        rng <<= 8 * k
        lower <<= 8 * k
        nbytes += k
        t = rng // total
        yield i, lower, rng, t, total, nbytes
        s = int(symbols[i])
        lower += int(counts[:s].sum()) * t
        rng = int(counts[s]) * t
        counts[s] += 1
        total += 1


def past_the_table(d, b, position):
    """Block b's stream with the target of one symbol at in-group position `position` past the table, then runs of 0xFF
    and of 0x00, then random bytes; None if no group from the 20th on leaves room behind the table there."""
    good, orig = d.good(b), d.orig[b]
    want = {16 * g + position for g in range(20, 40)}
    for i, lower, rng, t, total, nbytes in walk(good, max(want)):
        # the walk is the reference's: the undamaged stream's low lies inside the interval of the symbol it codes
        low = int.from_bytes(orig[4: 4 + nbytes].tobytes(), "big") - lower
        below = int(np.count_nonzero(good[:i] < good[i])) + int(good[i])  # cumulative count under symbol i
        mine = int(np.count_nonzero(good[:i] == good[i])) + 1
        assert below * t <= low < (below + mine) * t, (i, "the walk left the reference's interval")
        room = rng - total * t
        if i in want and room > 0:
            s = d.padded(b)
            code = lower + total * t + room // 2
            s[4: 4 + nbytes] = np.frombuffer(code.to_bytes(nbytes, "big"), np.uint8)
            at = 4 + nbytes
            for r, fill in enumerate((0xFF, 0x00, 0xFF, 0x00)):
                s[at + 48 * r: at + 48 * (r + 1)] = fill
            return s, i
    return None


@pytest.mark.parametrize("position", [0, 1, 15])
def test_target_past_the_table_among_valid_blocks(contexts, oracle, position):
    """One wave's 16 blocks, one of them damaged (in another quad for every position); every block's bytes and the
    call's status are what the oracle gives for each stream alone, and nothing outside the output is written
    (gpu_decode's guards)."""
    data = workloads.by_name("zipf", 16 * BLOCK, 40 + position)
    d = Damaged(oracle, data, BLOCK, rcx.CODER_ADAPTIVE, 40 + position)
    assert d.nblocks == 16
    b = (5, 0, 15)[(0, 1, 15).index(position)]
    made = past_the_table(d, b, position)
    assert made is not None
    stream, at_symbol = made
    d.damage(b, f"target past the table at symbol {at_symbol}", stream)
    # the reference's find() falls through with symbol 0 and count = total there, and the block goes on differently from its data
    ok, out = d.decode_one(b)
    assert ok and np.array_equal(out[:at_symbol], d.good(b)[:at_symbol]) and out[at_symbol] == 0
    assert not np.array_equal(out, d.good(b))
    for name in ("quads16", "default"):
        check_call(contexts[name], d, BLOCK, 0, (name, position))
