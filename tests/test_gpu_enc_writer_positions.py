"""The multi-wave encoders' writer wave (StagedWriter, csrc/rcx_mc.hpp; rcx_enc_mc5_k and rcx_enc_static3_k share it) keeps
its position as two running values, and forms the LDS address of a ring word by ORing the slot into the lane's address:
the output ring lies first in the workgroup's LDS, at a multiple of its 16 KiB.  (The arithmetic alone, at every position
and step: tests/test_enc_writer_positions_cpu.py.)

Every stream against the CPU oracle and decoded back, at the smallest shapes at which that can go wrong: the start of the
stream (the older word's slot is 63 until the fifth byte), blocks whose output wraps the 256-byte ring once and many
times, one lane in use up to more workgroups than CUs, the guarded pipeline, items, a single stream, and carries that
run back through the ring across a wrap -- inside the writer's window, through the ring walk, and past what the ring
keeps (the block is then coded again).  The same with the static coder.
"""
import numpy as np
import pytest

import carry_runs
from cpprcoder_amd import rcx, workloads
from gpu_support import check_blocks, check_items, ctx, oracle_streams  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MANY = 8250  # = 128 x 64 + 58: more workgroups than a device of up to 256 CUs has CUs, and a part-filled last workgroup
START = (16, 32, 48, 64)        # pipeline fill and drain; pos8 - 40 below zero at the stream's start
WRAPS = (272, 288, 512, 4096)   # the 256-byte ring wraps once ... sixteen times
COUNTS = (1, 3, 64, 65, MANY)
CODERS = (rcx.CODER_ADAPTIVE, rcx.CODER_STATIC)
CODER_IDS = ("adaptive", "static")


@pytest.mark.parametrize("coder", CODERS, ids=CODER_IDS)
@pytest.mark.parametrize("block", START + WRAPS)
def test_whole_blocks(ctx, oracle, block, coder):
    for i, nblocks in enumerate(COUNTS):
        check_blocks(ctx, oracle, workloads.by_name("uniform", block * nblocks, 2500 + i), block, coder=coder,
                     label=f"{nblocks} blocks")


@pytest.mark.parametrize("coder", CODERS, ids=CODER_IDS)
@pytest.mark.parametrize("block", START + WRAPS)
def test_guarded_pipeline(ctx, oracle, block, coder):
    """A ragged last block (block - 1 bytes at the most) beside whole ones, and a source one byte off alignment."""
    for i, tail in enumerate((1, 15, 17, 33)):
        for nblocks in (1, 3, 65):
            n = block * (nblocks - 1) + min(tail, block - 1)
            check_blocks(ctx, oracle, workloads.by_name("uniform", n, 2600 + i), block, coder=coder, label=f"{nblocks} blocks, tail {tail}")
    for nblocks in (1, 65):
        check_blocks(ctx, oracle, workloads.by_name("uniform", block * nblocks, 2700), block, coder=coder, src_offset=1,
                     label=f"{nblocks} blocks, source + 1")


@pytest.mark.parametrize("coder", CODERS, ids=CODER_IDS)
def test_items_of_unequal_length(ctx, oracle, coder):
    """Every lane with a length of its own: the rings of a workgroup wrap at different steps."""
    rs = np.random.RandomState(25)
    lengths = np.concatenate([[0, 1, 15, 16, 17, 255, 256, 257, 272], rs.randint(0, 1200, 400)]).astype(np.int64)
    rs.shuffle(lengths)
    data = workloads.by_name("uniform", int(lengths.sum()), 2800)
    ends = np.cumsum(lengths)
    items = [data[int(e - n): int(e)] for e, n in zip(ends, lengths)]
    check_items(ctx, items, oracle_streams(oracle, items, coder), coder=coder)


@pytest.mark.parametrize("n", [17, 300, 20000])
def test_single_stream(ctx, oracle, n):
    data = workloads.by_name("uniform", n, 2900 + n)
    status, want, size = oracle.adaptive_encode(data)
    st, rq, out = ctx.stream_encode(data)
    assert (st, rq) == tuple(status) == (0, 0) and out == want[:size]
    st, rq, back = ctx.stream_decode(out, n)
    assert st == 0 and back == data.tobytes()


# (run asked for, seed, first steered symbol, payload offset of the first zero, zeroes there): blocks of tests/carry_runs.py
# whose run of 0xFF bytes -- zeroes once the carry went through; the generator makes run .. run + 2 of them -- lies across
# payload byte 256, where the ring wraps, the byte the carry ends in on the other side.  Runs of 1 to 5 stay inside the
# writer's window or just leave it, 30 and 31 end in the ring walk (RCX_OUT_MARGIN is 32), 33 and 34 go past what the ring keeps.
CARRY_BLOCK = 1024
CARRY_RUNS = [(1, 50000, 250, 255, 2), (2, 50000, 250, 255, 3), (3, 50000, 250, 255, 4), (4, 50000, 250, 255, 4),
              (5, 50000, 250, 255, 6), (30, 50000, 236, 246, 31), (31, 50000, 236, 246, 32), (33, 50000, 236, 246, 34),
              (34, 50000, 236, 246, 35)]


def test_carry_runs_across_a_ring_wrap(ctx, oracle):
    parts = [carry_runs.carry_run_block(CARRY_BLOCK, run, seed, after) for run, seed, after, _, _ in CARRY_RUNS]
    slots, sizes = oracle.encode_blocks(np.concatenate(parts), CARRY_BLOCK)
    for b, (run, _, _, at, zeroes) in enumerate(CARRY_RUNS):  # (the inputs do what the table says: a slot is u32 size + payload)
        payload = slots[b, 4: int(sizes[b])]
        assert not payload[at: at + zeroes].any() and payload[at - 1] != 0 and payload[at + zeroes] != 0, f"run {run}"
        assert run <= zeroes <= run + 2 and at - 1 < 256 <= at + zeroes - 1, f"run {run}"
    # beside blocks without a run, 64 and more to a call: every lane of a workgroup, and a second workgroup
    for nblocks in (len(parts), 70):
        fill = [workloads.by_name("uniform", CARRY_BLOCK, 3000 + i) for i in range(nblocks - len(parts))]
        order = np.random.RandomState(nblocks).permutation(nblocks)
        blocks = parts + fill
        check_blocks(ctx, oracle, np.concatenate([blocks[i] for i in order]), CARRY_BLOCK, label=f"{nblocks} blocks")


def test_static_carry_runs(ctx, oracle):
    """The static coder's writer is the same: runs of every kind, wherever they fall in a block of four ring lengths."""
    block = 1024

    def make(run, i):
        for seed in range(50):
            try:
                return carry_runs.carry_run_block_static(block, run, 7000 + 100 * i + seed)
            except AssertionError:  # (no run with this seed: the next one)
                pass
        raise RuntimeError("no carry run found")

    parts = [make(run, i) for i, run in enumerate((1, 2, 3, 4, 5, 30, 31, 33, 34))]
    check_blocks(ctx, oracle, np.concatenate(parts), block, coder=rcx.CODER_STATIC)
