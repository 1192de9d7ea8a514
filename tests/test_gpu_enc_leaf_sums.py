"""The adaptive encoder's model waves (rcx_enc_mc5_k, csrc/rcx_mc.hpp) form their sums of a group as chains of 24-bit
multiply-adds (csrc/rcx_lane.hpp: rcx_pre4), and the leaf wave reads the symbol's count from LDS directly in front of the
symbol's own update, with the reads and updates running symbols ahead of the sums.  (The one-lane encoder, which codes a
block again after a long carry, takes the count as the difference of two such chains: rcx_pre4_sel4.)

What that depends on, every stream against the CPU oracle and decoded back: the pipeline's fill and drain at every depth,
counts past 16 bits, every position in a leaf group with large counts below it, a symbol that comes again within the
read-ahead (its count must hold every earlier bump and not its own), and the guarded pipeline, items and single streams.
(The arithmetic alone, for every count below 2^24: tests/test_enc_sums_cpu.py.)
"""
import numpy as np
import pytest

from cpprcoder_amd import rcx, workloads
from gpu_support import check_blocks, check_items, ctx, oracle_streams  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MANY = 8250  # = 128 x 64 + 58: more workgroups than a device of up to 256 CUs has CUs, and a part-filled last workgroup
BLOCKS = (16, 32, 48, 64, 4096)
COUNTS = (1, 3, 64, 65, 130, MANY)


@pytest.mark.parametrize("block", BLOCKS)
def test_fill_and_drain(ctx, oracle, block):
    """Whole blocks of 1, 2, 3, 4 and 256 chunks: the pipeline filling and draining at every depth, one lane in use, a
    part-filled last workgroup, more workgroups than CUs."""
    for i, nblocks in enumerate(COUNTS):
        check_blocks(ctx, oracle, workloads.by_name("uniform", block * nblocks, 2100 + i), block, label=f"{nblocks} blocks")


@pytest.mark.parametrize("symbol", [0, 3, 252, 255])
def test_counts_past_16_bits(ctx, oracle, symbol):
    """One 65536-byte block of one symbol: its count reaches 65537, at position 0 and 3 of the first and the last leaf group."""
    check_blocks(ctx, oracle, np.full(65536, symbol, np.uint8), 65536)


@pytest.mark.parametrize("group", [0, 21, 63])
@pytest.mark.parametrize("weights", [(8, 4, 2, 1), (1, 2, 4, 8)])
def test_one_leaf_group(ctx, oracle, group, weights):
    """Blocks drawn from one leaf group's four symbols alone: every position has up to three large counts below it."""
    block, nblocks = 4096, 65
    rs = np.random.RandomState(100 * group + weights[0])
    p = np.array(weights, np.float64) / sum(weights)
    data = (4 * group + rs.choice(4, size=block * nblocks, p=p)).astype(np.uint8)
    check_blocks(ctx, oracle, data, block, label=f"group {group}, weights {weights}")


def repeats(pattern, n):
    return np.resize(np.array(pattern, np.uint8), n)


@pytest.mark.parametrize("block", [48, 4096])
def test_symbol_again_within_the_read_ahead(ctx, oracle, block):
    """aaaa..., abab... with a and b in one leaf group, aabbaabb...: the count read for symbol s + 2 holds the bumps of s and
    s + 1 and not its own.  Several blocks to a call, each with its own pair."""
    nblocks = 65
    for name, shape in (("aaaa", (0,)), ("abab", (0, 1)), ("aabb", (0, 0, 1, 1))):
        blocks = []
        for b in range(nblocks):
            a = (37 * b + 5) % 256
            other = (a & ~3) | ((a + 1 + b % 3) & 3)  # another symbol of a's leaf group
            blocks.append(repeats([a if s == 0 else other for s in shape], block))
        check_blocks(ctx, oracle, np.concatenate(blocks), block, label=name)


@pytest.mark.parametrize("block", BLOCKS)
def test_guarded_pipeline_ragged_tail(ctx, oracle, block):
    """A ragged last block of 1, 15 or 17 bytes (block - 1 at the most) beside whole ones."""
    for i, tail in enumerate((1, 15, 17)):
        for nblocks in (1, 3, 65, 130):
            n = block * (nblocks - 1) + min(tail, block - 1)
            check_blocks(ctx, oracle, workloads.by_name("zipf", n, 2200 + i), block, label=f"{nblocks} blocks, tail {tail}")


@pytest.mark.parametrize("block", BLOCKS)
def test_guarded_pipeline_unaligned_source(ctx, oracle, block):
    """A source at + 1 and + 5 bytes: every workgroup takes the guarded pipeline."""
    for i, off in enumerate((1, 5)):
        for nblocks in (1, 65, 130):
            check_blocks(ctx, oracle, workloads.by_name("uniform", block * nblocks, 2300 + i), block, src_offset=off,
                         label=f"{nblocks} blocks, source + {off}")


def test_ragged_items(ctx, oracle):
    """2000 items of 0 .. 4096 bytes, 0, 1, 15, 16 and 17 among them: every lane with a length of its own."""
    rs = np.random.RandomState(21)
    lengths = np.concatenate([[0, 1, 15, 16, 17], rs.randint(0, 4097, 1995)]).astype(np.int64)
    rs.shuffle(lengths)
    data = workloads.by_name("zipf", int(lengths.sum()), 2400)
    ends = np.cumsum(lengths)
    items = [data[int(e - n): int(e)] for e, n in zip(ends, lengths)]
    check_items(ctx, items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE))


@pytest.mark.parametrize("n", [1, 17, 100003])
def test_single_stream(ctx, oracle, n):
    """rcx_stream_encode: one lane in use, the guarded pipeline unless the length is a multiple of 16."""
    data = workloads.by_name("zipf", n, 2500 + n)
    status, want, size = oracle.adaptive_encode(data)
    st, rq, out = ctx.stream_encode(data)
    assert (st, rq) == tuple(status) == (0, 0) and out == want[:size]
    st, rq, back = ctx.stream_decode(out, n)
    assert st == 0 and back == data.tobytes()
