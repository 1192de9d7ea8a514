"""The coders at the block counts, totals and alignments where a kernel or a launch shape changes (csrc/rcx_launch.hpp,
rcx_static.hpp, rcx_rans.hpp), every stream against the oracle and back.

* Launch shapes by block count: encode_lanes() doubles the blocks per workgroup of the multi-wave encoders behind
  cus x 1, 2, ... 32 blocks, decode_quads() the blocks per wave of the 4-lane decoders behind 4 cus x 1, 2, 4, 8, and the
  static encoder changes kernel at 32768 blocks.  gpu_support.shape_edges() lists those counts with both neighbours
  (tests/test_support_cpu.py holds the list to the formulas); all four coders run at each, with 16-byte blocks and a
  ragged last one -- seats, idle quads and the tail are all there, and the call stays small.
* Forced shapes: RCX_DEC_QUADS = 1 ... 16 for the static and the one-state rANS decoders at block counts that leave
  waves and workgroups part-filled.
* The static three-wave encoder takes 24-bit multiplies when every total of a wave is at least 256: whole blocks of
  240, 256 and 272 bytes.
* The rANS kernels' 8- and 16-byte paths: buffers 8 bytes behind a 16-byte border.

Measured on an MI355X (256 compute units), per test: the block-count tests 0.38 - 0.47 s at 32767 ... 32769 blocks (the
oracle's pass and the per-block compare included), 0.10 - 0.12 s around 8192 blocks, under 0.1 s below; every other test
of this file under 0.1 s; the 100 tests together 11 s.
"""
import numpy as np
import pytest

from cpprcoder_amd import rcx, workloads
from gpu_support import (CODERS, SHAPE_EDGE_IDS, Guarded, assert_same_blocks, check_blocks, context, ctx, gpu_decode,  # noqa: F401
                         gpu_encode, shape_edges)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CODER_IDS = {rcx.CODER_ADAPTIVE: "adaptive", rcx.CODER_STATIC: "static", rcx.CODER_RANS: "rans", rcx.CODER_RANS8: "rans8"}


def ragged(nblocks, block, last, workload, seed):
    """`nblocks` blocks of `workload` bytes, the last one `last` bytes long."""
    return workloads.by_name(workload, (nblocks - 1) * block + last, seed)


# ---- every edge count, every coder ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("coder", CODERS, ids=[CODER_IDS[c] for c in CODERS])
@pytest.mark.parametrize("edge", range(len(SHAPE_EDGE_IDS)), ids=SHAPE_EDGE_IDS)
def test_block_counts_where_a_launch_shape_changes(ctx, oracle, edge, coder):
    cus = torch.cuda.get_device_properties(0).multi_processor_count   # what rcx_ctx_create reads
    nblocks = shape_edges(cus)[edge]
    data = ragged(nblocks, 16, 1 + nblocks % 15, "zipf", nblocks)
    check_blocks(ctx, oracle, data, 16, coder=coder, threads=16, label=(SHAPE_EDGE_IDS[edge], nblocks, CODER_IDS[coder]))


# ---- forced shapes ---------------------------------------------------------------------------------------------------------
FORCED_CODERS = (rcx.CODER_STATIC, rcx.CODER_RANS)
FORCED_COUNTS = (1, 5, 17, 63, 65, 200)   # part-filled waves (1 ... 16 quads) and workgroups (4 waves) at every shape


@pytest.fixture(scope="module")
def forced_references(oracle):
    """(coder, count) -> (data, slots, sizes): 64-byte blocks, the last one ragged; the oracle's streams, made once."""
    out = {}
    for coder in FORCED_CODERS:
        for count in FORCED_COUNTS:
            data = ragged(count, 64, 1 + (7 * count) % 63, "canterbury" if coder == rcx.CODER_RANS else "zipf", 300 + count)
            out[coder, count] = (data, *oracle.encode_blocks(data, 64, coder=coder, threads=8))
    return out


@pytest.mark.parametrize("quads", [1, 2, 4, 8, 16])
def test_forced_blocks_per_wave(forced_references, quads):
    """rcx_dec_static_quad_k and rcx_dec_rans1_quad_k with `quads` blocks a wave whatever the count: idle seats in the
    last wave, idle waves in the last workgroup."""
    c = context({"RCX_DEC_QUADS": str(quads)})
    try:
        for (coder, count), (data, slots, sizes) in forced_references.items():
            label = (quads, CODER_IDS[coder], count)
            payload, offsets, _ = gpu_encode(c, data, 64, coder=coder)
            assert_same_blocks(payload, offsets, slots, sizes, label)
            back, st, _ = gpu_decode(c, payload, offsets, len(data), 64, coder=coder)
            assert st == 0 and np.array_equal(back, data), label
            if coder == rcx.CODER_STATIC:
                assert c.last_redo(count) == 0, label   # (the 4-lane kernel decoded them, not the pass behind it)
    finally:
        c.close()


# ---- the static encoder around a total of 256 ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def static_contexts(ctx):
    """The default context; the one-wave encoder; and 64 blocks a workgroup, where 130 blocks are two full workgroups and
    two blocks more.  (With fewer blocks than compute units the default shape is one block a workgroup: the 63 idle lanes
    of its waves have a total of 0, and `narrow` is never taken.)"""
    made = {"one wave": context({"RCX_ENC_VARIANT": "0"}), "64 lanes": context({"RCX_ENC_LANES": "64"})}
    yield {"default": ctx, **made}
    for c in made.values():
        c.close()


@pytest.mark.parametrize("workload", ["uniform", "runs"])
@pytest.mark.parametrize("block", [240, 256, 272])
def test_static_totals_around_256(static_contexts, oracle, block, workload):
    """rcx_enc_static3_k: `narrow = __all(total >= 256)` picks the 24-bit multiplies; at a total of exactly 256,
    range / 256 needs all 24 bits.  Whole blocks (total = block) from an aligned source, and once more with a last block
    of 100 bytes."""
    for last in (block, 100):
        data = ragged(130, block, last, workload, 10 * block + last)
        slots, sizes = oracle.encode_blocks(data, block, coder=rcx.CODER_STATIC, threads=8)
        for name, c in static_contexts.items():
            label = (name, block, last, workload)
            payload, offsets, _ = gpu_encode(c, data, block, coder=rcx.CODER_STATIC)
            assert_same_blocks(payload, offsets, slots, sizes, label)
            back, st, _ = gpu_decode(c, payload, offsets, len(data), block, coder=rcx.CODER_STATIC)
            assert st == 0 and np.array_equal(back, data), label


# ---- the rANS kernels 8 bytes behind a 16-byte border ------------------------------------------------------------------------
def test_an_offset_of_8_is_8_behind_a_border():
    assert Guarded(64, 8).view.data_ptr() % 16 == 8 and Guarded(64, 0).view.data_ptr() % 16 == 0


@pytest.mark.parametrize("coder", [rcx.CODER_RANS, rcx.CODER_RANS8], ids=["rans", "rans8"])
@pytest.mark.parametrize("block", [64, 4096])
def test_rans_buffers_8_behind_a_16_byte_border(ctx, oracle, block, coder):
    """A source that is 8-byte but not 16-byte aligned (by_eights without aligned16), a destination likewise (out8), and
    stream words that are even-aligned off a 16-byte border; each also with the other side on the border."""
    data = ragged(70, block, block // 3 + 5, "canterbury", block + coder)
    slots, sizes = oracle.encode_blocks(data, block, coder=coder, threads=8)
    for src_offset in (8, 0):
        payload, offsets, _ = gpu_encode(ctx, data, block, src_offset=src_offset, coder=coder)
        assert_same_blocks(payload, offsets, slots, sizes, (block, src_offset))
    for dst_offset, comp_offset in ((8, 0), (8, 8), (0, 0), (0, 8)):
        back, st, _ = gpu_decode(ctx, payload, offsets, len(data), block, dst_offset=dst_offset, comp_offset=comp_offset, coder=coder)
        assert st == 0 and np.array_equal(back, data), (block, dst_offset, comp_offset)
