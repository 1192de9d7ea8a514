"""The adaptive encoder's divisors (rcx_enc_mc5_k, rcx_mc.hpp; EncLane::arith_i): the arithmetic wave keeps a chunk's 16
multipliers and increments in registers, loaded from the quad decoder's table a chunk ahead, takes the shift once per
chunk, and folds the renormalising shift of the symbol before into the add of the increment.

The places that arrangement depends on -- block lengths around the totals that are powers of two (where the shift changes,
and the entries whose increment is 1), the largest ranges a total allows, the register reload at every chunk in the FULL and
in the guarded pipeline, items, a single stream -- every stream against the CPU oracle, and decoded back.  (The arithmetic
alone, over every total: tests/test_enc_divisors_cpu.py.)

A block shorter than a tail of 17 or 33 bytes takes the longest tail it has room for (block - 1).
"""
import numpy as np
import pytest

from cpprcoder_amd import rcx, workloads
from gpu_support import check_blocks, check_items, ctx, oracle_streams  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MANY = 8250  # = 128 x 64 + 58: 64 blocks a workgroup on a device of up to 256 CUs, and a part-filled last workgroup
BLOCKS = (16, 32, 48, 64, 80, 4096)
COUNTS = (1, 3, 64, 65, 130, MANY)


def lengths_around_powers_of_two(top):
    """Symbol counts i where the total 256 + i is a power of two, and next to them (either side of a chunk of 16): as
    tests/test_gpu_dec_divisors.py builds them."""
    out = []
    k = 9
    while (1 << k) - 256 <= top:
        edge = (1 << k) - 256
        out += [v for v in (edge - 17, edge - 16, edge - 1, edge, edge + 1, edge + 15, edge + 16, edge + 17) if 0 < v <= top]
        k += 1
    return out


def source(wl, n, seed):
    if wl == "repeat":
        return np.full(n, (seed * 37 + 5) % 256, np.uint8)
    return workloads.by_name(wl, n, seed)


@pytest.mark.parametrize("wl", ["uniform", "zipf", "repeat"])
def test_single_blocks_across_shift_changes(ctx, oracle, wl):
    """One block of every length around a power-of-two total: the last chunk straddles the change, ends on it, or is the
    first behind it."""
    block = 1 << 18
    for i, n in enumerate(lengths_around_powers_of_two(block)):
        check_blocks(ctx, oracle, source(wl, n, 77 + i), block, label=f"{wl}, {n} bytes")


@pytest.mark.parametrize("symbol", [0, 255])
def test_largest_ranges(ctx, oracle, symbol):
    """One bench-sized block of one symbol alone: its count is total - 255 at every symbol, the largest ranges there are."""
    check_blocks(ctx, oracle, np.full(65536, symbol, np.uint8), 65536)


@pytest.mark.parametrize("block", BLOCKS)
def test_full_pipeline(ctx, oracle, block):
    """Whole blocks of 1 .. 5 chunks and of 256: fill and drain, the reload at every chunk, one lane in use, part-filled
    workgroups and more than one workgroup."""
    for i, nblocks in enumerate(COUNTS):
        check_blocks(ctx, oracle, workloads.by_name("uniform", block * nblocks, 300 + i), block, label=f"{nblocks} blocks")


@pytest.mark.parametrize("block", BLOCKS)
def test_guarded_pipeline_ragged_tail(ctx, oracle, block):
    """A ragged last block: its workgroup takes the guarded pipeline, with whole blocks in the lanes beside it."""
    for i, tail in enumerate((1, 15, 17, 33)):
        for nblocks in COUNTS:
            n = block * (nblocks - 1) + min(tail, block - 1)
            check_blocks(ctx, oracle, workloads.by_name("zipf", n, 400 + i), block, label=f"{nblocks} blocks, tail {tail}")


@pytest.mark.parametrize("block", BLOCKS)
def test_guarded_pipeline_unaligned_source(ctx, oracle, block):
    """A source that is not 16-byte aligned: every workgroup takes the guarded pipeline."""
    for i, off in enumerate((1, 5)):
        for nblocks in COUNTS:
            check_blocks(ctx, oracle, workloads.by_name("uniform", block * nblocks, 500 + i), block, src_offset=off,
                         label=f"{nblocks} blocks, source + {off}")


@pytest.mark.parametrize("size,count", [(64, MANY), (4096, 65)])
def test_equal_items(ctx, oracle, size, count):
    # equal items, a multiple of 16 bytes at aligned addresses: the FULL pipeline; their streams are their blocks'
    data = workloads.by_name("zipf", size * count, size)
    slots, sizes = oracle.encode_blocks(data, size, threads=8)
    check_items(ctx, [data[i * size: (i + 1) * size] for i in range(count)], [slots[i, : int(sizes[i])] for i in range(count)])


def test_ragged_items(ctx, oracle):
    # 0 .. 4096 bytes: the guarded pipeline, every lane with a length of its own, lanes that end chunks before the others
    rs = np.random.RandomState(6)
    lengths = np.concatenate([[0, 1, 15, 16, 17, 4095, 4096], rs.randint(0, 4097, 2000)]).astype(np.int64)
    rs.shuffle(lengths)
    data = workloads.by_name("uniform", int(lengths.sum()), 99)
    ends = np.cumsum(lengths)
    items = [data[int(e - n): int(e)] for e, n in zip(ends, lengths)]
    check_items(ctx, items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE))


@pytest.mark.parametrize("n", [1, 17, 255, 257, (1 << 12) - 257, (1 << 12) - 255, 100003])
def test_single_stream(ctx, oracle, n):
    """rcx_stream_encode: one lane in use, lengths that are no multiple of 16, across shift changes."""
    data = workloads.by_name("zipf", n, n)
    status, want, size = oracle.adaptive_encode(data)
    st, rq, out = ctx.stream_encode(data)
    assert (st, rq) == tuple(status) == (0, 0) and out == want[:size]
    st, rq, back = ctx.stream_decode(out, n)
    assert st == 0 and back == data.tobytes()
