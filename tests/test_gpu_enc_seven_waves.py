"""The adaptive encoder's level-3 wave (rcx_enc_mc5_k): level 3 of the model is computed by a wave of its own
and reaches the arithmetic wave as a fifth value per symbol through a plane of LDS beside the ring.  The smallest shapes
at which that hand-over can go wrong -- the pipeline's fill and drain, the level's boundaries and largest sums, the
guarded pipeline, items, a single stream -- every stream against the CPU oracle, and decoded back.  Nothing here reads
/root/reference.

How many blocks a workgroup carries follows from the block count (rcx_launch.hpp:encode_lanes: one per workgroup up to
one workgroup per CU, 64 from 32 workgroups' worth per CU on): MANY blocks is enough for 64 a workgroup on a device of up
to 256 CUs, with a last workgroup that is part filled.
"""
import numpy as np
import pytest

from adaptive_cases import LEVEL3_CASES, level3_block
from cpprcoder_amd import rcx
from gpu_support import check_blocks, check_items, ctx, oracle_streams  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MANY = 8250  # = 128 x 64 + 58
EDGES = np.array([0, 63, 64, 127, 128, 191, 192, 255], np.uint8)  # both sides of every level-3 boundary


def symbols(name, n, seed=0):
    """n bytes: 'uniform', 'edges' (only the symbols on either side of a level-3 boundary) or 'quarter0' .. 'quarter3'
    (confined to one quarter of the alphabet: one level-3 sum takes every update above it)."""
    rs = np.random.RandomState(1000 + seed)
    if name == "uniform":
        return rs.randint(0, 256, n).astype(np.uint8)
    if name == "edges":
        return EDGES[rs.randint(0, len(EDGES), n)]
    return (64 * int(name[-1]) + rs.randint(0, 64, n)).astype(np.uint8)


SETS = ("edges", "quarter0", "quarter1", "quarter2", "quarter3")


@pytest.mark.parametrize("block", [16, 32, 48, 64, 4096])
def test_pipeline_fill_and_drain(ctx, oracle, block):
    """Full blocks of 1 .. 4 chunks and of 256: the level-3 plane is written in step k and read in step k + 1, from the
    first chunk to the last, with one lane in use, part-filled workgroups and more than one workgroup."""
    for i, nblocks in enumerate((1, 3, 64, 65, 130, MANY)):
        check_blocks(ctx, oracle, symbols("uniform", block * nblocks, i), block)


@pytest.mark.parametrize("name", SETS)
def test_level3_boundaries(ctx, oracle, name):
    for i, (block, nblocks) in enumerate(((48, 3), (64, MANY), (4096, 65))):
        check_blocks(ctx, oracle, symbols(name, block * nblocks, i), block)


@pytest.mark.parametrize("case", LEVEL3_CASES)
def test_largest_level3_sums(ctx, oracle, case):
    """One bench-sized block.  Of symbol 0 alone: all three sums grow with every symbol, to 65536 + 192.  Of symbol 255
    alone: the sum below the last quarter is handed over with every symbol.  Of symbol 0 with a 255 now and then, and as
    the last symbol: the largest sums there can be, up to 192 + 65535, go through the plane."""
    check_blocks(ctx, oracle, level3_block(case), 65536)  # (the builder: tests/adaptive_cases.py)


@pytest.mark.parametrize("name", SETS)
def test_guarded_pipeline(ctx, oracle, name):
    """A ragged last block (its workgroup takes the guarded pipeline, the lanes beside it with whole blocks) and a source
    that is not 16-byte aligned (every workgroup does)."""
    for i, tail in enumerate((1, 15, 17, 33)):
        for block, nblocks in ((48, 3), (64, MANY)):
            check_blocks(ctx, oracle, symbols(name, block * (nblocks - 1) + tail, i), block)
    for i, off in enumerate((1, 5)):
        for block, nblocks in ((64, MANY), (4096, 65)):
            check_blocks(ctx, oracle, symbols(name, block * nblocks, 10 + i), block, src_offset=off)
        check_blocks(ctx, oracle, symbols(name, 64 * (MANY - 1) + 17, 20 + i), 64, src_offset=off)


@pytest.mark.parametrize("name", ("uniform", "edges", "quarter3"))
def test_items(ctx, oracle, name):
    # equal items, a multiple of 16 bytes at aligned addresses: the FULL pipeline; their streams are their blocks'
    for size, count in ((64, MANY), (4096, 65)):
        data = symbols(name, size * count, size)
        slots, sizes = oracle.encode_blocks(data, size, threads=8)
        check_items(ctx, [data[i * size: (i + 1) * size] for i in range(count)], [slots[i, : int(sizes[i])] for i in range(count)])
    # items of differing sizes: the guarded pipeline, every lane with a length of its own
    lengths = np.tile(np.array([1, 15, 16, 17, 33, 48, 64, 100, 333, 4096, 5000], np.int64), MANY // 11)
    np.random.RandomState(5).shuffle(lengths)
    data = symbols(name, int(lengths.sum()), 99)
    ends = np.cumsum(lengths)
    items = [data[int(e - n): int(e)] for e, n in zip(ends, lengths)]
    check_items(ctx, items, oracle_streams(oracle, items, rcx.CODER_ADAPTIVE))


def test_single_stream(ctx, oracle):
    """rcx_stream_encode: one lane in use, a length that is no multiple of 16."""
    for i, (name, n) in enumerate((("edges", 333), ("quarter0", 201), ("quarter3", 777), ("uniform", 500), ("edges", 16), ("quarter2", 17))):
        data = symbols(name, n, i)
        status, want, size = oracle.adaptive_encode(data)
        st, rq, out = ctx.stream_encode(data)
        assert (st, rq) == tuple(status) == (0, 0) and out == want[:size]
        st, rq, back = ctx.stream_decode(out, n)
        assert st == 0 and back == data.tobytes()
