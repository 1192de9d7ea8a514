"""The adaptive quad decoder where a node's counts borrow: round 2 of rcx_dec_quad_k keeps the counts negated in LDS and
takes the borrows of rem - Q * t from the high words of 64-bit multiply-adds -- the symbol is the lane's last one plus
three of them, the owner word (what ds_add puts on the count, what masks the output byte) is made of two (DESIGN 3.4,
round 7).

Round trips on inputs that sit on every boundary of round 2 -- the first and last count of each lane of a quad, in the
first and the last node; values that alternate across a lane boundary and across a node's ends; a count that grows to
2^18 while t shrinks --, a single stream (the one-wave instantiation), an items call, and damaged streams whose target
lies past the table, so that the scratch row -- parked output bytes by then -- is read as counts.  The reference is the
oracle: its streams, and what it decodes from each damaged stream alone (include/rcx.h, "Damaged streams").
"""
import numpy as np
import pytest

from adaptive_walk import past_the_table
from cpprcoder_amd import rcx, workloads
from gpu_support import Damaged, assert_same_blocks, check_call, check_items, context, gpu_decode, gpu_encode, oracle_streams

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BLOCK = 4096
RAGGED = 1237  # the last block: 77 groups of 16 and 5 symbols one by one
SLOTS = (0, 3, 4, 7, 8, 11, 12, 15)  # the first and the last count of every lane
REPEATED = tuple(16 * node + slot for node in (0, 15) for slot in SLOTS)
NODE = 9  # the node the alternating values lie in
PAIRS = tuple((16 * NODE + a, 16 * NODE + b) for a, b in ((3, 4), (7, 8), (11, 12), (0, 15)))  # lane boundaries, the node's ends
DRAWN = ("zipf", "uniform", "runs")
KINDS = len(REPEATED) + len(PAIRS) + len(DRAWN)  # 23
FIRST_KINDS = (0, 12)  # 17 or 18 blocks from kind 0 and from kind 12: every kind in each shape


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


def buffer_of(nblocks, first_kind):
    """nblocks blocks of BLOCK bytes and a ragged one, block b of kind (first_kind + b) mod KINDS."""
    parts = [block_of((first_kind + b) % KINDS, BLOCK if b < nblocks else RAGGED, 700 + b) for b in range(nblocks + 1)]
    return np.concatenate(parts)


def test_the_two_shapes_carry_every_kind():
    for nblocks in (16, 17):
        assert {(f + b) % KINDS for f in FIRST_KINDS for b in range(nblocks + 1)} == set(range(KINDS))


@pytest.mark.parametrize("first_kind", FIRST_KINDS)
@pytest.mark.parametrize("nblocks", [16, 17])
def test_round_trips_on_the_boundaries_of_round_two(contexts, oracle, nblocks, first_kind):
    data = buffer_of(nblocks, first_kind)
    slots, sizes = oracle.encode_blocks(data, BLOCK, threads=8)
    for name, ctx in contexts.items():
        payload, offsets, _ = gpu_encode(ctx, data, BLOCK)
        assert_same_blocks(payload, offsets, slots, sizes)
        back, st, _ = gpu_decode(ctx, payload, offsets, len(data), BLOCK)
        assert st == rcx.OK, name
        assert np.array_equal(back, data), (name, int(np.nonzero(back != data)[0][0]) // BLOCK)


@pytest.mark.parametrize("byte", [0, 255])
def test_one_large_block_of_one_byte(contexts, oracle, byte):
    """2^18 symbols of one value: its negated count falls to -2^18 while t falls to range / 2^18."""
    n = 1 << 18
    data = np.full(n, byte, np.uint8)
    slots, sizes = oracle.encode_blocks(data, n)
    for name, ctx in contexts.items():
        payload, offsets, _ = gpu_encode(ctx, data, n)
        assert_same_blocks(payload, offsets, slots, sizes)
        back, st, _ = gpu_decode(ctx, payload, offsets, n, n)
        assert st == rcx.OK and np.array_equal(back, data), name


def test_single_stream(contexts, oracle):
    """rcx_stream_decode: the one-wave instantiation, one quad in use, whole groups and a tail."""
    data = buffer_of(1, len(REPEATED))[: BLOCK + 5]  # a pair block and five symbols one by one
    data = np.concatenate([data, workloads.by_name("zipf", 1237, 9)])
    status, want, size = oracle.adaptive_encode(data)
    assert tuple(status) == (0, 0)
    for name, ctx in contexts.items():
        st, rq, back = ctx.stream_decode(want[:size], len(data))
        assert (st, rq) == (0, 0) and back == data.tobytes(), name


def test_three_unequal_items(contexts, oracle):
    """The item geometry: three items of unequal lengths, so the second and third begin at unaligned addresses."""
    lengths = (1237, BLOCK + 3, 333)
    items = [block_of(k, n, 900 + k) for k, n in zip((len(REPEATED) + 1, KINDS - 3, 7), lengths)]
    want = oracle_streams(oracle, items, rcx.CODER_ADAPTIVE)
    for name, ctx in contexts.items():
        check_items(ctx, items, want, label=name)


# Damaged streams: adaptive_walk.past_the_table makes a target past the table, from the 20th group on, when the scratch
# row the decoder then reads as counts already holds parked output bytes.
@pytest.mark.parametrize("position", [0, 1, 15])
def test_scratch_row_read_as_counts_among_valid_blocks(contexts, oracle, position):
    """One wave's 16 blocks, one of them damaged (in another quad for every position); every block's bytes and the
    call's status are what the oracle gives for each stream alone, and nothing outside the output is written
    (gpu_decode's guards)."""
    data = workloads.by_name("zipf", 16 * BLOCK, 70 + position)
    d = Damaged(oracle, data, BLOCK, rcx.CODER_ADAPTIVE, 70 + position)
    assert d.nblocks == 16
    b = (9, 3, 12)[(0, 1, 15).index(position)]
    made = past_the_table(d, b, position)
    assert made is not None
    stream, at_symbol = made
    assert at_symbol >= 320 and at_symbol % 16 == position
    d.damage(b, f"target past the table at symbol {at_symbol}", stream)
    # the reference's find() falls through with symbol 0 and count = total there, and the block goes on differently from its data
    ok, out = d.decode_one(b)
    assert ok and np.array_equal(out[:at_symbol], d.good(b)[:at_symbol]) and out[at_symbol] == 0
    assert not np.array_equal(out, d.good(b))
    for name in ("quads16", "default"):
        check_call(contexts[name], d, BLOCK, 0, (name, position))
