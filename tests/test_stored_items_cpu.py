"""Stored items as far as they go without a GPU: the header against stored_items.EXPORTS and the built library, the worked
example of include/rcx_stored_items.h, the numpy mirror on the CPU oracle's streams of all four coders, the sizes the design
states for the tensor buffers, and RCXJ version 2: its bytes, its parser and what that refuses."""
import os
import re
import struct

import numpy as np
import pytest

import stored_items_cases as sic
from cpprcoder_amd import container, layout, rcx, stored, stored_items

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def declared_symbols(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rcx_[a-z0-9_]+)\s*\(", text)))


def test_header_exports_and_library_agree():
    from cpprcoder_amd import build, planes, predict, stats, typed_items
    build.build()
    names = declared_symbols("rcx_stored_items.h")
    assert len(names) == 2 and set(names) == set(stored_items.EXPORTS), (names, stored_items.EXPORTS)
    for name in names:
        assert getattr(stored_items.lib(), name).argtypes is not None
    assert '#include "rcx_stored.h"' in open(os.path.join(ROOT, "include", "rcx_stored_items.h")).read()
    # every other header is what it was
    assert len(declared_symbols("rcx.h")) == 57 and len(declared_symbols("rcx_stored.h")) == 4
    assert len(rcx.EXPORTS) == 57 and len(stored.EXPORTS) == 4 and len(planes.EXPORTS) == 4 and len(predict.EXPORTS) == 4
    assert len(stats.EXPORTS) == 4 and len(typed_items.EXPORTS) == 6
    assert rcx.lib().rcx_version() == 300
    others = set(rcx.EXPORTS) | set(stored.EXPORTS) | set(planes.EXPORTS) | set(predict.EXPORTS) | set(stats.EXPORTS) | set(typed_items.EXPORTS)
    assert not set(stored_items.EXPORTS) & others
    assert all(h in build.HEADERS for h in ("rcx_stored_items.hpp", "rcx_stored_items_api.hpp"))
    assert any(h.endswith("rcx_stored_items.h") for h in build.HEADERS)
    assert build.HEADERS.index("rcx_stored_items.hpp") > build.HEADERS.index("rcx_stored.hpp")


# ---- the mirror ----------------------------------------------------------------------------------------------------------------
def test_the_headers_worked_example():
    """Four items of 16, 0, 8 and 40 bytes whose streams have 20, 0, 8 and 21: stored, never, the tie, kept."""
    src = np.arange(64, dtype=np.uint8)
    comp = np.arange(100, 149, dtype=np.uint8)
    soffs, coffs = [0, 16, 16, 24, 64], [0, 20, 20, 28, 49]
    mixed, moffs, flags = stored_items.mix_items_numpy(src, soffs, comp, coffs, 0)
    assert flags.tolist() == [1, 0, 1, 0] and moffs.tolist() == [0, 16, 16, 24, 45]
    assert np.array_equal(mixed, np.concatenate([src[0:16], src[16:24], comp[28:49]]))
    mixed, moffs, flags = stored_items.mix_items_numpy(src, soffs, comp, coffs, 32768)
    assert flags.tolist() == [1, 0, 1, 1] and moffs.tolist() == [0, 16, 16, 24, 64] and np.array_equal(mixed, src)
    # the empty item is not stored under the largest gain either, and its entry of the stream table is not looked at
    odd = [0, 20, 7, 28, 49]
    mixed, moffs, flags = stored_items.mix_items_numpy(src, soffs, comp, odd, 65535)
    assert flags.tolist() == [1, 0, 1, 1] and moffs.tolist() == [0, 16, 16, 24, 64]
    # items that begin past the front of the buffer
    mixed, moffs, flags = stored_items.mix_items_numpy(src, [16, 24, 64], comp, [20, 28, 49], 0)
    assert flags.tolist() == [1, 0] and moffs.tolist() == [0, 8, 29] and np.array_equal(mixed, np.concatenate([src[16:24], comp[28:49]]))
    m, o, f = stored_items.mix_items_numpy(b"", [0], b"", [0])
    assert len(m) == 0 and o.tolist() == [0] and len(f) == 0
    m, o, f = stored_items.mix_items_numpy(b"", [0, 0, 0], b"", [0, 0, 0], 65535)
    assert len(m) == 0 and o.tolist() == [0, 0, 0] and f.tolist() == [0, 0]
    for bad in (([0, 16], [0, 5, 9]), ([0, 16, 8], [0, 5, 9]), ([0, 16, 80], [0, 5, 9]), ([0, 16, 24], [0, 9, 5]), ([0, 16, 24], [0, 9, 50])):
        with pytest.raises(ValueError):
            stored_items.mix_items_numpy(src, bad[0], comp, bad[1])
    with pytest.raises(ValueError):
        stored_items.mix_items_numpy(src, soffs, comp, coffs, 65536)


def decode_with_oracle(oracle, mixed, moffs, flags, items, coder):
    lengths = [len(x) for x in items]

    def decode(stream, length, i):
        if length == 0:
            return np.zeros(0, np.uint8)
        slots = np.zeros((1, len(stream) + 64), np.uint8)
        slots[0, : len(stream)] = stream
        out, ok = oracle.decode_blocks(slots, np.array([len(stream)], np.uint32), length, length, coder=coder)
        assert ok, i
        return out

    return stored.unmix_numpy(mixed, moffs, flags, lengths, decode)


@pytest.mark.parametrize("coder", sic.CODERS)
def test_mix_items_numpy_on_the_oracles_streams(oracle, coder):
    items = sic.ragged_items()
    src = np.concatenate(items)
    soffs = sic.offsets_of([len(x) for x in items])
    payload, offsets = sic.oracle_item_streams(oracle, items, coder)
    mixed, moffs, flags = stored_items.mix_items_numpy(src, soffs, payload, offsets, 0)
    print(coder, "".join("S" if f else "c" for f in flags), int(offsets[-1]), int(moffs[-1]))
    assert flags.any() and not flags.all(), "both kinds of item"
    assert int(moffs[-1]) == len(mixed) <= len(src) and len(mixed) <= len(payload)
    for i, x in enumerate(items):
        got = mixed[int(moffs[i]): int(moffs[i + 1])]
        coded = payload[int(offsets[i]): int(offsets[i + 1])]
        assert flags[i] == (len(x) > 0 and len(coded) >= len(x)), i
        assert np.array_equal(got, x if flags[i] else coded), i
        assert len(x) or (flags[i] == 0 and len(got) == 0)
    assert np.array_equal(decode_with_oracle(oracle, mixed, moffs, flags, items, coder), src)
    # a larger gain stores no less; the largest stores every item that has bytes
    for gain in (256, 65535):
        more = stored_items.mix_items_numpy(src, soffs, payload, offsets, gain)[2]
        assert bool((more >= flags).all())
    assert more.tolist() == [int(len(x) > 0) for x in items]


# ---- the sizes the design states ---------------------------------------------------------------------------------------------
def test_the_tensor_buffers_at_64_kib(oracle):
    text, soffs = sic.typed_sub_items(65536)
    assert len(text) == 4 << 20 and len(soffs) == 65
    slots, sizes = oracle.encode_blocks(text, 65536, coder=0, threads=8)
    payload, offsets = oracle.compact(slots, sizes)
    mixed, moffs, flags = stored_items.mix_items_numpy(text, soffs, payload, offsets, 0)
    assert (int(offsets[-1]), int(moffs[-1]), int(flags.sum())) == (2072650, 2071707, 8)
    assert int(stored_items.mix_items_numpy(text, soffs, payload, offsets, 256)[2].sum()) == 20
    # the eight-state rANS coder: a container that was larger than its input
    slots, sizes = oracle.encode_blocks(text, 65536, coder=3, threads=8)
    payload, offsets = oracle.compact(slots, sizes)
    mixed, moffs, flags = stored_items.mix_items_numpy(text, soffs, payload, offsets, 0)
    print("rANS8 stored:", int(flags.sum()), "of", len(flags))
    assert int(offsets[-1]) == 4878440 > len(text) >= int(moffs[-1]) == 3461628
    assert int(flags.sum()) == 45  # (the count that gives those two totals)


def test_records_of_16_bytes_do_not_expand(oracle):
    items = sic.zipf_batch(200, 16)
    src = np.concatenate(items)
    soffs = sic.offsets_of([16] * 200)
    for coder in sic.CODERS:
        payload, offsets = sic.oracle_item_streams(oracle, items, coder)
        mixed, moffs, flags = stored_items.mix_items_numpy(src, soffs, payload, offsets, 0)
        assert int(offsets[-1]) > 3200 and bool(flags.all()) and int(moffs[-1]) == 3200 and np.array_equal(mixed, src), coder


# ---- RCXJ version 2 ------------------------------------------------------------------------------------------------------------
LENGTHS, WIDTHS, PREDS = [23, 0, 7, 16], [4, 2, 1, 8], [2, 0, 0, 1]   # sub-items: 5 5 5 8 | 0 0 | 7 | 2 2 2 2 2 2 2 2
SUB = [5, 5, 5, 8, 0, 0, 7] + [2] * 8
FLAGS = [1, 0, 1, 1, 0, 0, 0] + [1] * 8       # bits 0 2 3 | 7 .. 14: bytes 0x8D 0x7F
SIZES = [5, 9, 5, 8, 0, 0, 11] + [2] * 8      # a stored sub-item's stream is the sub-item
OFFS = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint64)
PAYLOAD = bytes(range(int(OFFS[-1])))
BITMAP = b"\x8d\x7f"
CRCS = np.arange(100, 115, dtype=np.uint32)
TABLES = struct.pack("<4Q", *LENGTHS) + bytes(WIDTHS) + bytes(PREDS) + OFFS.astype("<u8").tobytes()


def blob_j(stored=FLAGS, crcs=None, directory=b"", offs=OFFS):
    return container.typed_items_header_bytes(1, LENGTHS, WIDTHS, PREDS, offs, crcs, directory, stored) + PAYLOAD


def test_rcxj_version_2_byte_for_byte():
    assert layout.TYPED_ITEMS_VERSION == 1 and layout.TYPED_ITEMS_VERSION_STORED == 2 and container.TYPED_ITEMS_VERSION_STORED == 2
    assert blob_j() == struct.pack("<4sBBHQQQ", b"RCXJ", 2, 1, 4, 4, 15, 0) + TABLES + BITMAP + PAYLOAD
    c = container.parse_typed_items(blob_j())
    assert c["stored"].dtype == bool and c["stored"].tolist() == [bool(f) for f in FLAGS] and c["crcs"] is None and c["flags"] == container.FLAG_STORED
    assert list(c["sub_lengths"]) == SUB and np.array_equal(c["offsets"], OFFS) and bytes(c["payload"]) == PAYLOAD
    # with checksums and a directory: the bitmap, then the CRC table, then the directory
    assert blob_j(crcs=CRCS, directory=b"hello") == (struct.pack("<4sBBHQQQ", b"RCXJ", 2, 1, 6, 4, 15, 5) + TABLES + BITMAP + CRCS.astype("<u4").tobytes()
                                                     + b"hello" + PAYLOAD)
    c = container.parse_typed_items(blob_j(crcs=CRCS, directory=b"hello"))
    assert c["flags"] == 6 and c["stored"].tolist() == [bool(f) for f in FLAGS] and np.array_equal(c["crcs"], CRCS) and c["directory"] == b"hello"


def test_without_a_stored_sub_item_the_header_is_todays():
    plain = np.concatenate([[0], np.cumsum([9, 9, 9, 12, 0, 0, 11] + [6] * 8)]).astype(np.uint64)
    for crcs in (None, CRCS):
        today = container.typed_items_header_bytes(1, LENGTHS, WIDTHS, PREDS, plain, crcs, b"d")
        assert today[4] == 1 and today[6] == (2 if crcs is not None else 0)
        assert container.typed_items_header_bytes(1, LENGTHS, WIDTHS, PREDS, plain, crcs, b"d", None) == today
        assert container.typed_items_header_bytes(1, LENGTHS, WIDTHS, PREDS, plain, crcs, b"d", np.zeros(15, np.uint8)) == today
        assert container.parse_typed_items(today + bytes(int(plain[-1]))).get("stored") is None
    empty = container.typed_items_header_bytes(0, [], [], None, [0], None, b"", [])
    assert empty == container.typed_items_header_bytes(0, [], [], None, [0])


def with_byte(blob, at, value):
    b = bytearray(blob)
    b[at] = value
    return bytes(b)


def test_what_the_parser_refuses():
    blob = blob_j()
    at = 32 + len(TABLES)  # the bitmap's first byte
    assert container.parse_typed_items(blob)["stored"].sum() == 11
    same_text = [with_byte(blob, 6, 0), with_byte(blob, 6, 2),     # version 2 without bit 2
                 with_byte(blob, 4, 1),                            # bit 2 in version 1
                 with_byte(blob, 6, 12), with_byte(blob, 6, 5), with_byte(blob, 7, 1),  # a flag nobody knows beside it
                 with_byte(blob, 4, 3)]                            # there is no version 3
    for damaged in same_text:
        with pytest.raises(container.ContainerError, match="unsupported container version, coder or flags"):
            container.parse_typed_items(damaged)
    bad = [with_byte(blob, at + 1, 0xFF),                          # a padding bit
           with_byte(with_byte(blob, at, 0), at + 1, 0),           # an empty bitmap
           with_byte(blob, at, 0x8F),                              # sub-item 1: stored, and 9 bytes for its 5
           with_byte(blob, at, 0xCD),                              # sub-item 6: stored, and 11 bytes for its 7
           with_byte(blob, at, 0x9D), with_byte(blob, at, 0xAD),   # a stored empty sub-item
           blob[:at + 1], blob[:at], blob[:at - 3],               # a truncated bitmap, a truncated table
           blob + b"x", blob[:-1]]
    for k, damaged in enumerate(bad):
        with pytest.raises(container.ContainerError):
            container.parse_typed_items(damaged)
            print("not refused:", k)
    # a version 1 container with the version byte or the flag changed stays refused
    v1 = container.typed_items_header_bytes(1, LENGTHS, WIDTHS, PREDS, OFFS) + PAYLOAD
    container.parse_typed_items(v1)
    for damaged in (with_byte(v1, 4, 2), with_byte(v1, 6, 4), with_byte(v1, 6, 6)):
        with pytest.raises(container.ContainerError, match="unsupported container version, coder or flags"):
            container.parse_typed_items(damaged)
    # what the header function refuses
    wrong = OFFS.copy()
    wrong[1:] += np.uint64(1)  # sub-item 0, stored, with 6 bytes for its 5
    for kw in (dict(stored=[1] * 14), dict(stored=[1] * 16),       # one flag per sub-item
               dict(stored=[1] * 15),                              # an empty sub-item, and streams of another length
               dict(stored=[0, 0, 0, 0, 1] + [0] * 10),            # a stored empty sub-item alone
               dict(stored=[0, 1] + [0] * 13),                     # 9 bytes for 5
               dict(offs=wrong)):
        with pytest.raises(container.ContainerError):
            blob_j(**kw)
    # the item container has no such version
    iblob = bytearray(container.item_header_bytes(0, [100, 0, 7], [0, 60, 60, 75]) + bytes(75))
    iblob[4], iblob[6] = 2, 4
    with pytest.raises(container.ContainerError):
        container.parse_items(bytes(iblob))


def test_the_option_is_checked_before_a_gpu_is_needed():
    for bad in (1, 1.0, -0.5, "yes", 2, [0.5]):
        with pytest.raises(container.ContainerError):
            container.pack_typed_items([b"abc"], widths=1, stored=bad)
        with pytest.raises(container.ContainerError):
            container.pack_tensors({"t": np.zeros(4, np.float32)}, stored=bad)
    # nothing to code: today's containers, and no GPU
    assert container.pack_typed_items([b"", b""], widths=1, stored=True) == container.pack_typed_items([b"", b""], widths=1)
    assert container.pack_tensors({"t": np.zeros((0, 4), np.float32)}, stored=0.25) == container.pack_tensors({"t": np.zeros((0, 4), np.float32)})
    assert "widths=1" in container.pack_items.__doc__ and "widths=1" in layout.__doc__
