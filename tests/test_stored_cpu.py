"""Stored blocks as far as they go without a GPU: the header against stored.EXPORTS and the built library, the rule of
include/rcx_stored.h at its pins, its numpy mirror on the CPU oracle's streams of all four coders -- blocks that no coder
shrinks beside blocks that every coder does, and the byte planes of fp32 data -- and the two version-3 containers: their bytes,
their parsers and what those refuse."""
import os
import re
import struct

import numpy as np
import pytest

import stored_cases as sc
from cpprcoder_amd import container, rcx, stored

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rcx_stored.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, predict, stats
    build.build()
    names = declared_symbols()
    assert len(names) == 4 and set(names) == set(stored.EXPORTS), (names, stored.EXPORTS)
    for name in names:
        assert getattr(stored.lib(), name).argtypes is not None
    assert '#include "rcx.h"' in open(os.path.join(ROOT, "include", "rcx_stored.h")).read()
    # rcx.h, rcx_planes.h, rcx_predict.h and rcx_stats.h are what they were
    assert len(rcx.EXPORTS) == 57 and len(planes.EXPORTS) == 4 and len(predict.EXPORTS) == 4 and len(stats.EXPORTS) == 4
    assert rcx.lib().rcx_version() == 300
    assert not set(stored.EXPORTS) & (set(rcx.EXPORTS) | set(planes.EXPORTS) | set(predict.EXPORTS) | set(stats.EXPORTS))
    assert all(h in build.HEADERS for h in ("rcx_stored.hpp", "rcx_stored_api.hpp")) and any(h.endswith("rcx_stored.h") for h in build.HEADERS)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def test_the_rule_at_its_pins():
    for length in (1, 16, 100, 65536, rcx.MAX_BLOCK):
        assert stored.is_stored(length, length, 0) and not stored.is_stored(length - 1, length, 0)  # a tie is stored
    assert stored.is_stored(65280, 65536, 256) and not stored.is_stored(65279, 65536, 256)
    assert all(stored.is_stored(coded, 16, 65535) for coded in range(1, 40)) and not stored.is_stored(0, 16, 65535)
    # RCX_MAX_BLOCK: len * gain is below 2^40, nowhere near the 64 bits it is computed in
    top = rcx.MAX_BLOCK
    share = (top * 65535) >> 16
    assert share == top - 256 and stored.is_stored(top - share, top, 65535) and not stored.is_stored(top - share - 1, top, 65535)
    huge = np.array([1 << 62, 0], np.uint64)
    assert stored.is_stored(huge, np.array([top, top], np.uint64), 65535).tolist() == [True, False]
    # arrays and integers agree
    coded = np.arange(65270, 65290)
    assert stored.is_stored(coded, np.full(20, 65536), 256).tolist() == [stored.is_stored(int(c), 65536, 256) for c in coded]
    for bad in (-1, 65536):
        with pytest.raises(ValueError):
            stored.is_stored(1, 2, bad)


def test_gain_q16():
    assert stored.gain_q16(True) == 0 and stored.gain_q16(0) == 0 and stored.gain_q16(0.0) == 0
    assert stored.gain_q16(256 / 65536) == 256 and stored.gain_q16(0.5) == 32768 and stored.gain_q16(0.9999999) == 65535
    assert stored.gain_q16(1e-9) == 0
    for bad in (False, None, 1, 1.0, -0.1, "0.5", 2):
        with pytest.raises(ValueError):
            stored.gain_q16(bad)


# ---- the mirror on the oracle's streams --------------------------------------------------------------------------------------
def unmix_with_oracle(oracle, mixed, moffs, flags, n, block, coder):
    lengths = stored.block_lengths(n, block)

    def decode(stream, length, b):
        slots = np.zeros((1, len(stream) + 64), np.uint8)
        slots[0, : len(stream)] = stream
        out, ok = oracle.decode_blocks(slots, np.array([len(stream)], np.uint32), block, length, coder=coder)
        assert ok, b
        return out

    return stored.unmix_numpy(mixed, moffs, flags, lengths, decode)


@pytest.mark.parametrize("block", (4096, 65536))
@pytest.mark.parametrize("coder", sc.CODERS)
def test_mix_numpy_on_the_oracles_streams(oracle, coder, block):
    x = sc.mixed_bytes(block)
    assert len(x) == 6 * block - 7
    payload, offsets = sc.oracle_streams(oracle, x, block, coder)
    mixed, moffs, flags = stored.mix_numpy(x, block, payload, offsets, 0)
    print(coder, block, sc.pattern(flags), np.diff(offsets.astype(np.int64)).tolist(), int(moffs[-1]))
    if block == 65536 or coder != 3:  # (eight-state rANS at 4096: its 1032-byte table and the doubled constant block leave nothing to keep)
        assert flags.any() and not flags.all(), "both kinds of block"
    assert sc.pattern(flags) == sc.PATTERNS[block][coder]
    assert int(moffs[-1]) == len(mixed) <= len(x) and int(moffs[-1]) <= int(offsets[-1])
    if coder == 3:
        assert flags[3] == 1 and int(offsets[4] - offsets[3]) > 2 * block  # the block of one repeated byte, doubled by the coder
    lengths = stored.block_lengths(len(x), block)
    for b in range(6):
        got = mixed[int(moffs[b]): int(moffs[b + 1])]
        want = x[b * block: b * block + int(lengths[b])] if flags[b] else payload[int(offsets[b]): int(offsets[b + 1])]
        assert np.array_equal(got, want), b
    assert np.array_equal(unmix_with_oracle(oracle, mixed, moffs, flags, len(x), block, coder), x)
    # a larger gain stores no less; the largest stores everything
    for gain in (256, 65535):
        more = stored.mix_numpy(x, block, payload, offsets, gain)[2]
        assert bool((more >= flags).all())
    assert bool(more.all())


def test_small_blocks_are_nearly_all_stored(oracle):
    for block in (16, 100):
        for coder in sc.CODERS:
            x = sc.mixed_bytes(block)
            mixed, moffs, flags = stored.mix_numpy(x, block, *sc.oracle_streams(oracle, x, block, coder), 0)
            assert int(flags.sum()) >= (3 if (block, coder) == (100, 0) else 6) and len(mixed) <= len(x)


def test_fp32_planes(oracle):
    """Sizes of the four planes, low mantissa first: adaptive 65653 65654 65395 22230, static 66036 66037 65778 22455,
    rANS 66546 66548 66289 22967, rANS8 66570 66570 66312 23002."""
    y = sc.fp32_planes()
    for coder in sc.CODERS:
        payload, offsets = sc.oracle_streams(oracle, y, 65536, coder)
        flags = stored.mix_numpy(y, 65536, payload, offsets, 0)[2]
        print(coder, np.diff(offsets.astype(np.int64)).tolist(), sc.pattern(flags))
        assert flags[0] == 1 and flags[1] == 1 and flags[3] == 0
        if coder == 0:
            assert flags[2] == 0 and stored.mix_numpy(y, 65536, payload, offsets, 256)[2].tolist() == [1, 1, 1, 0]
            assert np.array_equal(unmix_with_oracle(oracle, *stored.mix_numpy(y, 65536, payload, offsets, 256), len(y), 65536, 0), y)


def test_the_mirrors_refusals():
    x = np.zeros(40, np.uint8)
    with pytest.raises(ValueError):
        stored.mix_numpy(x, 16, np.zeros(10, np.uint8), [0, 5, 10])  # three blocks, two streams
    with pytest.raises(ValueError):
        stored.unmix_numpy(np.zeros(15, np.uint8), [0, 15], [1], [16], None)  # a stored block one byte short
    assert len(stored.unmix_numpy(b"", [0], None, [], None)) == 0
    m, o, f = stored.mix_numpy(b"", 16, b"", [0])
    assert len(m) == 0 and o.tolist() == [0] and len(f) == 0


# ---- containers ------------------------------------------------------------------------------------------------------------
N3, BLOCK = 3 * 4096 - 7, 4096
OFFS = np.array([0, 4096, 4196, 4196 + 4089], np.uint64)  # blocks 0 and 2 stored, block 1 a stream of 100 bytes
FLAGS = np.array([1, 0, 1], np.uint8)
CRCS = np.array([11, 22, 33], np.uint32)
PAYLOAD = bytes(int(OFFS[-1]))


def test_rcxb_version_3_byte_for_byte():
    h = container.header_bytes(2, BLOCK, N3, OFFS, 0, None, FLAGS)
    assert h == struct.pack("<4sBBHIQQ", b"RCXB", 3, 2, 4, BLOCK, N3, 3) + OFFS.astype("<u8").tobytes() + b"\x05"
    c = container.parse(h + PAYLOAD)
    assert (c["coder"], c["flags"], c["block"], c["n"], c["nblocks"]) == (2, container.FLAG_STORED, BLOCK, N3, 3)
    assert c["stored"].dtype == bool and c["stored"].tolist() == [True, False, True] and c["crcs"] is None and len(c["payload"]) == len(PAYLOAD)
    assert np.array_equal(c["offsets"], OFFS)
    # with checksums: the bitmap, then the CRC table
    h = container.header_bytes(0, BLOCK, N3, OFFS, 0, CRCS, FLAGS)
    assert h == struct.pack("<4sBBHIQQ", b"RCXB", 3, 0, 6, BLOCK, N3, 3) + OFFS.astype("<u8").tobytes() + b"\x05" + CRCS.astype("<u4").tobytes()
    c = container.parse(h + PAYLOAD)
    assert c["flags"] == 6 and c["stored"].tolist() == [True, False, True] and np.array_equal(c["crcs"], CRCS)
    # with the block sort's flag: the lengths are those of the bytes the coder saw
    n = 3 * 32768 - 2
    offs4 = np.array([0, 32768, 32778, 32788, 32788 + 2], np.uint64)  # m = n + 4: three whole blocks and one of 2 bytes
    h = container.header_bytes(1, 32768, n, offs4, container.FLAG_BLKSORT, None, [1, 0, 0, 1])
    c = container.parse(h + bytes(int(offs4[-1])))
    assert h[4] == 3 and c["flags"] == 5 and c["stored"].tolist() == [True, False, False, True]
    # nine blocks: two bytes of bitmap, the padding zero
    offs9 = np.arange(10, dtype=np.uint64) * np.uint64(16)
    h = container.header_bytes(0, 16, 9 * 16, offs9, 0, None, np.ones(9))
    assert h[-2:] == b"\xff\x01" and bool(container.parse(h + bytes(144))["stored"].all())


def test_rcxt_version_3_byte_for_byte():
    for pred in (0, 1, 2):
        h = container.typed_header_bytes(2, BLOCK, N3, 4, OFFS, None, pred, FLAGS)
        assert h == (struct.pack("<4sBBHIQQB7s", b"RCXT", 3, 2, 4, BLOCK, N3, 3, 4, bytes([pred]) + bytes(6)) + OFFS.astype("<u8").tobytes() + b"\x05")
        c = container.parse_typed(h + PAYLOAD)
        assert (c["coder"], c["flags"], c["block"], c["n"], c["nblocks"], c["width"], c["pred"]) == (2, 4, BLOCK, N3, 3, 4, pred)
        assert c["stored"].tolist() == [True, False, True] and c["crcs"] is None
    h = container.typed_header_bytes(0, BLOCK, N3, 8, OFFS, CRCS, 2, FLAGS)
    assert h == (struct.pack("<4sBBHIQQB7s", b"RCXT", 3, 0, 6, BLOCK, N3, 3, 8, b"\x02" + bytes(6)) + OFFS.astype("<u8").tobytes() + b"\x05"
                 + CRCS.astype("<u4").tobytes())
    c = container.parse_typed(h + PAYLOAD)
    assert c["flags"] == 6 and c["pred"] == 2 and c["stored"].tolist() == [True, False, True] and np.array_equal(c["crcs"], CRCS)


def test_without_a_stored_block_the_headers_are_todays():
    plain = np.array([0, 100, 200, 251], np.uint64)
    for crcs in (None, CRCS):
        today = container.header_bytes(2, BLOCK, N3, plain, 0, crcs)
        assert container.header_bytes(2, BLOCK, N3, plain, 0, crcs, None) == today
        assert container.header_bytes(2, BLOCK, N3, plain, 0, crcs, np.zeros(3, np.uint8)) == today and today[4] == (2 if crcs is not None else 1)
        assert container.parse(today + bytes(251))["stored"] is None
        for pred in (0, 1):
            today = container.typed_header_bytes(2, BLOCK, N3, 4, plain, crcs, pred)
            assert container.typed_header_bytes(2, BLOCK, N3, 4, plain, crcs, pred, [0, 0, 0]) == today and today[4] == (2 if pred else 1)
            assert container.parse_typed(today + bytes(251))["stored"] is None
    empty = container.header_bytes(0, 65536, 0, np.zeros(1, np.uint64), 0, None, np.zeros(0, np.uint8))
    assert empty == container.header_bytes(0, 65536, 0, np.zeros(1, np.uint64)) and container.parse(empty)["stored"] is None


def with_byte(blob, at, value):
    b = bytearray(blob)
    b[at] = value
    return bytes(b)


def test_what_the_parsers_refuse():
    for header, parse, fixed in ((container.header_bytes(2, BLOCK, N3, OFFS, 0, None, FLAGS), container.parse, 28),
                                 (container.typed_header_bytes(2, BLOCK, N3, 4, OFFS, None, 0, FLAGS), container.parse_typed, 36)):
        blob = header + PAYLOAD
        at = fixed + 8 * 4  # the bitmap's byte
        assert parse(blob)["stored"].tolist() == [True, False, True]
        bad = [with_byte(blob, 6, 0), with_byte(blob, 6, 2),      # version 3 without bit 2
               with_byte(blob, 4, 1), with_byte(blob, 4, 2),      # bit 2 in versions 1 and 2
               with_byte(blob, 6, 12),                            # a flag nobody knows beside it
               with_byte(blob, at, 0x0D), with_byte(blob, at, 0x85),  # a padding bit
               with_byte(blob, at, 0),                            # an empty bitmap
               with_byte(blob, at, 7), with_byte(blob, at, 2),    # block 1 is not 4096 bytes long: stored, its offsets are not len_b apart
               blob[:at], blob[: at - 3],                 # a truncated bitmap, a truncated table
               blob + b"x", blob[:-1]]
        for damaged in bad:
            with pytest.raises(container.ContainerError):
                parse(damaged)
    # the ragged last block: stored means its own length, not the block size
    wrong = np.array([0, 4096, 4196, 4196 + 4096], np.uint64)
    with pytest.raises(container.ContainerError):
        container.header_bytes(2, BLOCK, N3, wrong, 0, None, FLAGS)
    with pytest.raises(container.ContainerError):
        container.typed_header_bytes(2, BLOCK, N3, 4, wrong, None, 0, FLAGS)
    for bad_flags in ([1, 0], [1, 0, 1, 0]):  # one flag per block
        with pytest.raises(container.ContainerError):
            container.header_bytes(2, BLOCK, N3, OFFS, 0, None, bad_flags)
    with pytest.raises(container.ContainerError):
        container.header_bytes(2, BLOCK, N3, OFFS, container.FLAG_STORED)  # the flag without the bitmap
    # no blocks, so no stored block: version 3 of an empty container is refused
    empty = bytearray(container.header_bytes(0, 65536, 0, np.zeros(1, np.uint64)))
    empty[4], empty[6] = 3, 4
    with pytest.raises(container.ContainerError):
        container.parse(bytes(empty))
    # an item container has no version 3
    iblob = bytearray(container.item_header_bytes(0, [100, 0, 7], [0, 60, 60, 75]) + bytes(75))
    iblob[4], iblob[6] = 3, 4
    with pytest.raises(container.ContainerError):
        container.parse_items(bytes(iblob))


def test_the_refusals_from_before_still_hold():
    offs = np.array([0, 100, 200, 251], np.uint64)
    v2 = container.header_bytes(0, BLOCK, N3, offs, 0, CRCS) + bytes(251)
    v1 = container.header_bytes(0, BLOCK, N3, offs) + bytes(251)
    t2 = container.typed_header_bytes(0, BLOCK, N3, 4, offs, None, 1) + bytes(251)
    t1 = container.typed_header_bytes(0, BLOCK, N3, 4, offs, CRCS) + bytes(251)
    for blob, parse in ((v2, container.parse), (v1, container.parse), (t2, container.parse_typed), (t1, container.parse_typed)):
        parse(blob)
        for damaged in (with_byte(blob, 4, 3), with_byte(blob, 6, blob[6] | 4)):  # the version byte set to 3; flag 4 in versions 1 and 2
            with pytest.raises(container.ContainerError):
                parse(damaged)


def test_the_option_is_checked_before_a_gpu_is_needed():
    for bad in (1, 1.0, -0.5, "yes", 2, [0.5]):
        with pytest.raises(container.ContainerError):
            container.pack(b"abc", stored=bad)
        with pytest.raises(container.ContainerError):
            container.pack_typed(np.zeros(4, np.int32), stored=bad)
    # nothing to code: today's empty container
    assert container.pack_typed(np.zeros(0, np.int32), stored=True) == container.pack_typed(np.zeros(0, np.int32))


def test_command_line_takes_stored():
    from cpprcoder_amd.__main__ import parser
    ap = parser()
    assert ap.parse_args(["c", "in", "out"]).stored is None
    assert ap.parse_args(["c", "--stored", "--crc", "in", "out"]).stored is True
    assert ap.parse_args(["c", "--stored", "0.004", "in", "out"]).stored == 0.004
    assert ap.parse_args(["t", "--planes", "4", "--stored", "0.25", "f"]).stored == 0.25
    assert ap.parse_args(["t", "--blksort", "--stored", "--", "f"]).stored is True
    for argv in (["c", "--stored", "1", "in", "out"], ["c", "--stored", "-0.1", "in", "out"], ["d", "--stored", "in", "out"], ["t", "--stored", "1.5", "f"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
