"""The shared test support (tests/gpu_support.py) held to its contract, on CPU tensors: every "writes nothing outside
its buffer" claim of the GPU tests rests on Guarded.check failing when it should, their launch shapes on knobs leaving the
environment as it found it, and their parity claims on the two comparisons."""
import os

import numpy as np
import pytest

from gpu_support import (GUARD, SHAPE_EDGE_IDS, Guarded, assert_same_blocks, assert_same_items, chunk_blocks, decode_quads, encode_lanes,
                         knobs, shape_edges)

SIZES, OFFSETS = (0, 1, 33), (0, 15)


def guarded(size, offset, invert=False):
    return Guarded(size, offset, np.arange(size, dtype=np.uint8), salt=2, invert=invert, device="cpu")


@pytest.mark.parametrize("invert", [False, True])
def test_an_untouched_buffer_passes(invert):
    for size in SIZES:
        for offset in OFFSETS:
            g = guarded(size, offset, invert)
            assert g.view.numel() == size and g.view.tolist() == list(range(size))
            assert g.tensor.numel() == GUARD + offset + size + GUARD
            g.check(0)
            g.check(size)
            g.view.fill_(0)  # the call wrote all it may
            g.check(size)


def changed(g, position, written):
    """check(written) after one byte at `position` (relative to the buffer) changed -> the AssertionError's text."""
    g.tensor[g.at + position] ^= 0x40
    with pytest.raises(AssertionError) as e:
        g.check(written, "dst")
    return str(e.value)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("size", SIZES)
def test_one_changed_byte_outside_what_may_be_written_fails(size, offset):
    for written in sorted({0, size // 2, size}):
        for position in (-1, -(GUARD + offset), written, size + GUARD - 1):
            msg = changed(guarded(size, offset), position, written)
            assert msg.startswith(f"dst: byte {position} changed") and f"the {written} bytes" in msg, msg
    if size:  # an input: none of its bytes may change
        for position in (0, size - 1):
            assert f"byte {position} changed" in changed(guarded(size, offset), position, 0)


def test_the_lowest_changed_byte_is_named():
    g = guarded(33, 15)
    g.tensor[g.at + 40] ^= 1
    assert "byte 20 changed" in changed(g, 20, 10)
    g.tensor[g.at - 3] ^= 1
    with pytest.raises(AssertionError, match="byte -3 changed"):
        g.check(10)


def test_the_pattern_is_nonzero_and_differs_by_salt_and_inversion():
    images = {}
    for salt in (1, 2):
        for invert in (False, True):
            t = Guarded(1000, 3, salt=salt, invert=invert, device="cpu").tensor.numpy()
            assert t.min() >= 1, (salt, invert)  # (251 + 1 at the most, so the complement is nonzero too)
            images[salt, invert] = t
    assert np.array_equal(images[1, True], ~images[1, False])
    keys = list(images)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert np.count_nonzero(images[a] != images[b]) > 900, (a, b)


class Boom(Exception):
    pass


@pytest.mark.parametrize("fail", [False, True])
def test_knobs_restore_the_environment(monkeypatch, fail):
    monkeypatch.setenv("RCX_T_SET", "before")
    monkeypatch.setenv("RCX_T_CLEARED", "kept")
    monkeypatch.delenv("RCX_T_UNSET", raising=False)
    monkeypatch.delenv("RCX_T_CLEARED_UNSET", raising=False)
    whole = dict(os.environ)
    try:
        with knobs({"RCX_T_SET": "inside", "RCX_T_UNSET": "1"}, clear=("RCX_T_CLEARED", "RCX_T_CLEARED_UNSET")):
            assert os.environ["RCX_T_SET"] == "inside" and os.environ["RCX_T_UNSET"] == "1"
            assert "RCX_T_CLEARED" not in os.environ and "RCX_T_CLEARED_UNSET" not in os.environ
            if fail:
                raise Boom
    except Boom:
        assert fail
    assert dict(os.environ) == whole
    # a variable both cleared and set is set inside, and back to what it was afterwards
    with knobs({"RCX_T_CLEARED": "2"}, clear=("RCX_T_CLEARED",)):
        assert os.environ["RCX_T_CLEARED"] == "2"
    assert dict(os.environ) == whole


def test_chunk_blocks_restates_host_chunk_blocks():
    """csrc/rcx_host.hpp host_chunk_blocks(), by hand: 2048 (encode) or 4096 (decode) blocks, at least 16 MiB worth, doubled
    until there are at most 2048 chunks, then equal chunks, rounded up to a multiple of 64."""
    for (block, decode, nblocks), want in {
        (4096, True, 100): 4096,            # one chunk: the floor of 16 MiB / 4096 itself
        (4096, False, 100): 4096,           # (the encoder's 2048 is below that floor)
        (65536, False, 100): 2048,          # the floor is 256 blocks: the defaults stand
        (65536, True, 100): 4096,
        (16, True, 1): 1 << 20,             # 16 MiB of 16-byte blocks
        (4096, True, 9092): 3072,           # 3 chunks of 4096 -> 3031 each -> the next multiple of 64
        (4096, False, 22785): 3840,         # 6 chunks -> 3798 each -> 3840
        (65536, False, 4273): 1472,         # 3 chunks of 2048 -> 1425 each -> 1472
        (65536, True, 16384): 4096,         # 4 equal chunks exactly
        (1 << 20, True, 1 << 23): 4096,     # 2048 chunks: the most there may be
        (1 << 20, True, (1 << 23) + 1): 8192,  # one block more: 8192 a chunk, 1025 chunks of 8185 -> 8192
    }.items():
        assert chunk_blocks(block, decode, nblocks) == want, (block, decode, nblocks)


@pytest.mark.parametrize("cus", [256, 304])
def test_shape_edges_sit_on_every_change_of_launch_shape(cus):
    """csrc/rcx_launch.hpp encode_lanes() / decode_quads(), by hand, and the counts tests/test_gpu_launch_shapes.py walks:
    one block more than each multiple changes the shape, so a list without m + 1 would miss the change."""
    edges = shape_edges(cus)
    assert len(edges) == len(SHAPE_EDGE_IDS) == 21 and len(set(SHAPE_EDGE_IDS)) == 21
    for k, quads in ((1, 1), (2, 2), (4, 4), (8, 8)):
        m = 4 * cus * k
        assert (decode_quads(m - 1, cus), decode_quads(m, cus), decode_quads(m + 1, cus)) == (quads, quads, 2 * quads), m
        assert {m - 1, m, m + 1} <= set(edges)
    for k in (1, 2, 4, 8, 16, 32):
        m = cus * k
        assert (encode_lanes(m, cus), encode_lanes(m + 1, cus)) == (k, 2 * k), m
        assert encode_lanes(m - 1, cus) == k or k == 1
        assert {m - 1, m, m + 1} <= set(edges)
    assert decode_quads(1, cus) == encode_lanes(1, cus) == 1
    assert decode_quads(1 << 20, cus) == 16 and encode_lanes(1 << 20, cus) == 64          # the caps
    assert {32767, 32768, 32769} <= set(edges)
    assert edges == sorted(edges) or cus * 32 > 32767    # (in ascending order where the device is no larger than 1023 CUs)


def test_shape_edges_of_256_compute_units():
    edges = shape_edges(256)
    assert {1025, 8193, 32768} <= set(edges) and edges[:4] == [255, 256, 257, 511] and min(shape_edges(1)) == 1
    assert [decode_quads(n, 256) for n in (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)] == [1, 2, 2, 4, 4, 8, 8, 16]
    assert [encode_lanes(n, 256) for n in (256, 257, 8192, 8193, 32768)] == [1, 2, 32, 64, 64]
    # neither power-of-two rounding nor the cap is taken for granted: 3 workgroups' worth rounds up to 4
    assert encode_lanes(3 * 256, 256) == 4 and decode_quads(3 * 1024, 256) == 4 and decode_quads(5 * 1024, 256) == 8


def four_blocks():
    sizes = np.array([5, 7, 3, 6], np.uint32)
    slots = np.arange(4 * 16, dtype=np.uint8).reshape(4, 16) + 1
    streams = [slots[b, : int(sizes[b])] for b in range(4)]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return np.concatenate(streams), offsets, slots, sizes, streams


def test_the_comparisons_fail_when_they_should():
    payload, offsets, slots, sizes, streams = four_blocks()
    assert_same_blocks(payload, offsets, slots, sizes)
    assert_same_items(payload, offsets, streams)
    # an item of length 0 has no stream
    assert_same_items(payload, np.insert(offsets, 2, offsets[2]), streams[:2] + [None] + streams[2:])
    # a size mismatch: a byte moves from block 1 to block 2
    moved = offsets.copy()
    moved[2] -= 1
    with pytest.raises(AssertionError, match="sizes differ"):
        assert_same_blocks(payload, moved, slots, sizes)
    with pytest.raises(AssertionError, match="sizes"):
        assert_same_items(payload, moved, streams)
    with pytest.raises(AssertionError, match="sizes"):
        assert_same_items(payload, offsets, streams[:2] + [None] + streams[3:])
    # one byte of a middle block differs
    for at, b in ((int(offsets[2]), 2), (int(offsets[2]) - 1, 1)):
        bad = payload.copy()
        bad[at] ^= 1
        with pytest.raises(AssertionError, match=f"here: block {b} differs"):
            assert_same_blocks(bad, offsets, slots, sizes, "here")
        with pytest.raises(AssertionError, match=f"here: item {b} differs"):
            assert_same_items(bad, offsets, streams, "here")


# ---- tests/resumable_cases.py: what the GPU tests of the resumable coders take for granted about their inputs -------------
def test_a_constant_piece_ends_at_the_halving():
    import resumable_cases as rc
    from golden_cases import LONG_ADAPTIVE, NO_HALVING
    assert rc.H == NO_HALVING == (1 << 24) - 256 and NO_HALVING % 1_048_560 == 0 and rc.HALVING_PIECE == 1_048_560
    assert rc.LONG_UNIFORM in LONG_ADAPTIVE and rc.LONG_MIN_ZIPF in LONG_ADAPTIVE
    sizes = rc.around_halving(NO_HALVING + 5000)
    assert sizes == [NO_HALVING - 1, 1, 1, 4999] and sum(sizes) == NO_HALVING + 5000
    assert rc.constant(10, 4) == [4, 4, 2] and rc.split(b"abcdefghij", [4, 4, 2]) == [b"abcd", b"efgh", b"ij"]
    assert sum(rc.uneven(311_564)) == 311_564 and rc.uneven(311_564)[:5] == [100_000, 1, 1, 70_000, 8]


def test_the_carry_input_outgrows_the_facades_guess(oracle):
    import resumable_cases as rc
    data = rc.carry_input()
    assert len(data) == rc.CARRY_N
    (st, rq), sink, sizes = oracle.adaptive_encode_trace(data, rc.CARRY_PIECE)
    jumps = np.diff(sizes)
    assert (st, rq) == (0, 0) and int(jumps.max()) > 3 * 64 + 4096 == rc.FACADE_ROOM
    assert int(np.count_nonzero(jumps > rc.FACADE_ROOM)) == 1
    # the writer restated in resumable_cases agrees with the oracle about where the run ends, and how
    j = rc.carrying_symbol(data)
    assert j // rc.CARRY_PIECE == int(np.argmax(jumps))
    assert b"\x00" * (rc.CARRY_RUN - 1) in sink and b"\xff" * rc.CARRY_RUN not in sink


def test_the_altered_piece_does_not_carry(oracle):
    import resumable_cases as rc
    data = rc.carry_input()
    altered, j = rc.without_the_carry(data)
    assert len(altered) == len(data) and np.array_equal(altered[:j], data[:j]) and altered[j] != data[j]
    long_runs = [e for e in rc.writer_events(altered) if e[1] >= rc.CARRY_RUN]
    assert len(long_runs) == 1 and long_runs[0][0] == j and not long_runs[0][2]  # the run ends in symbol j, by a smaller byte
    assert b"\xff" * rc.CARRY_RUN in oracle.adaptive_encode(altered)[1]


def test_the_launch_loop_input_is_long_and_codes_small(oracle):
    import resumable_cases as rc
    v = rc.loop_input()
    assert len(v) == rc.LOOP_N == 2_621_440 == 5 * rc.CHUNK // 2 and int(v.max()) == 3
    assert len(oracle.adaptive_encode(v)[1]) < 1_000_000
    assert [-(-rc.LOOP_N // cap) for cap in rc.LOOP_CAPS + (rc.LOOP_ONE_CALL,)] == [3, 3, 3, 2, 1]
    kinds = [(k, len(b)) for k, b, _ in rc.interleaved_inputs()]
    assert [k for k, _ in kinds] == ["dec", "enc", "dec", "enc"] and all(20_000 <= n <= 70_000 for _, n in kinds)
