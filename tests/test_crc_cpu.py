"""Checksums as far as they go without a GPU: the version-2 headers of both containers, what stays version 1 byte for
byte, what is refused, the exception's place, the exports and the command line."""
import struct
import zlib

import numpy as np
import pytest

from cpprcoder_amd import container

CRC_SYMBOLS = ("rcx_crc32_blocks_device", "rcx_crc32_items_device", "rcx_crc32_verify_blocks_device", "rcx_crc32_verify_items_device",
               "rcx_crc32_blocks", "rcx_crc32_items")


def block_blob(crcs, flags=0):
    offs = np.array([0, 100, 250, 251], np.uint64)
    return container.header_bytes(0, 4096, 3 * 4096 - 7, offs, flags, crcs) + bytes(251), offs


def test_block_header_version_2_round_trips():
    crcs = np.array([0xCBF43926, 0, 0xFFFFFFFF], np.uint32)
    blob, offs = block_blob(crcs)
    assert blob[4] == 2 and struct.unpack_from("<H", blob, 6)[0] == container.FLAG_CRC32 == 2
    assert blob[28 + 8 * 4: 28 + 8 * 4 + 12] == crcs.astype("<u4").tobytes()  # the table follows the offsets
    c = container.parse(blob)
    assert (c["coder"], c["block"], c["n"], c["nblocks"], c["flags"]) == (0, 4096, 3 * 4096 - 7, 3, container.FLAG_CRC32)
    assert c["crcs"].dtype == np.uint32 and np.array_equal(c["crcs"], crcs)
    assert np.array_equal(c["offsets"], offs) and len(c["payload"]) == 251
    # with the block sort's flag beside it
    n = 3 * 32768 - 2
    offs4 = np.array([0, 10, 20, 30, 40], np.uint64)
    c = container.parse(container.header_bytes(1, 32768, n, offs4, container.FLAG_BLKSORT, np.arange(4, dtype=np.uint32)) + bytes(40))
    assert c["flags"] == container.FLAG_BLKSORT | container.FLAG_CRC32 and np.array_equal(c["crcs"], np.arange(4))
    # no data: no blocks, an empty table
    c = container.parse(container.header_bytes(0, 65536, 0, np.zeros(1, np.uint64), 0, np.zeros(0, np.uint32)))
    assert c["nblocks"] == 0 and c["crcs"] is not None and len(c["crcs"]) == 0


def test_item_header_version_2_round_trips():
    lengths = np.array([100, 0, 7, 70_000], np.uint64)
    offs = np.array([0, 60, 60, 75, 40_000], np.uint64)
    crcs = np.array([1, 0, zlib.crc32(b"abcdefg"), 0xDEADBEEF], np.uint32)
    blob = container.item_header_bytes(2, lengths, offs, crcs) + bytes(40_000)
    assert blob[4] == 2 and struct.unpack_from("<H", blob, 6)[0] == 2
    c = container.parse_items(blob)
    assert (c["coder"], c["nitems"]) == (2, 4) and len(c["payload"]) == 40_000
    assert np.array_equal(c["lengths"], lengths) and np.array_equal(c["offsets"], offs)
    assert c["crcs"].dtype == np.uint32 and np.array_equal(c["crcs"], crcs)
    c = container.parse_items(container.item_header_bytes(0, [], [0], np.zeros(0, np.uint32)))
    assert c["nitems"] == 0 and len(c["crcs"]) == 0


def test_without_checksums_the_headers_are_version_1_byte_for_byte():
    offs = np.array([0, 100, 250, 251], np.uint64)
    h = container.header_bytes(3, 4096, 3 * 4096 - 7, offs)
    assert h == struct.pack("<4sBBHIQQ", b"RCXB", 1, 3, 0, 4096, 3 * 4096 - 7, 3) + offs.astype("<u8").tobytes()
    assert h == container.header_bytes(3, 4096, 3 * 4096 - 7, offs, 0, None)
    assert container.parse(h + bytes(251))["crcs"] is None
    lengths, ioffs = np.array([5, 0, 9], np.uint64), np.array([0, 20, 20, 31], np.uint64)
    ih = container.item_header_bytes(1, lengths, ioffs)
    assert ih == struct.pack("<4sBBHQ", b"RCXI", 1, 1, 0, 3) + lengths.astype("<u8").tobytes() + ioffs.astype("<u8").tobytes()
    assert ih == container.item_header_bytes(1, lengths, ioffs, None)
    assert container.parse_items(ih + bytes(31))["crcs"] is None


def test_refused_headers():
    crcs = np.array([1, 2, 3], np.uint32)
    blob, _ = block_blob(crcs)
    plain, _ = block_blob(None)
    table_end = 28 + 8 * 4 + 12
    bad = bytearray(blob)
    struct.pack_into("<H", bad, 6, 0)                    # version 2 without the flag
    v2 = bytearray(plain)
    v2[4] = 2                                            # a version-1 blob whose version byte says 2
    v1 = bytearray(plain)
    v1[6] = 2                                            # a version-1 blob with the flag
    v3 = bytearray(blob)
    v3[4] = 3
    unknown = bytearray(blob)
    unknown[6] |= 4                                      # a flag nobody knows beside the CRC bit
    for damaged in (bytes(bad), bytes(v2), bytes(v1), bytes(v3), bytes(unknown), blob + b"x", blob[:-1], blob[: table_end - 1],
                    blob[: table_end - 5], blob[: 28 + 8 * 4]):  # a trailing byte, a short payload, a truncated CRC table
        with pytest.raises(container.ContainerError):
            container.parse(damaged)
    with pytest.raises(container.ContainerError):
        block_blob(np.array([1, 2], np.uint32))         # one checksum per block
    with pytest.raises(container.ContainerError):
        block_blob(None, container.FLAG_CRC32)          # the flag without the table
    lengths, offs = np.array([100, 0, 7], np.uint64), np.array([0, 60, 60, 75], np.uint64)
    iblob = container.item_header_bytes(0, lengths, offs, crcs) + bytes(75)
    iplain = container.item_header_bytes(0, lengths, offs) + bytes(75)
    itable_end = 16 + 8 * 3 + 8 * 4 + 12
    noflag = bytearray(iblob)
    struct.pack_into("<H", noflag, 6, 0)
    iv2 = bytearray(iplain)
    iv2[4] = 2
    iv1 = bytearray(iplain)
    iv1[6] = 2
    for damaged in (bytes(noflag), bytes(iv2), bytes(iv1), iblob + b"x", iblob[:-1], iblob[: itable_end - 1], iblob[: itable_end - 12]):
        with pytest.raises(container.ContainerError):
            container.parse_items(damaged)
    with pytest.raises(container.ContainerError):
        container.item_header_bytes(0, lengths, offs, np.zeros(4, np.uint32))
    with pytest.raises(container.ContainerError):        # the two containers still do not read each other's files
        container.parse(iblob)
    with pytest.raises(container.ContainerError):
        container.parse_items(blob)


def test_checksum_error_is_a_container_error():
    assert issubclass(container.ChecksumError, container.ContainerError) and issubclass(container.ChecksumError, ValueError)
    e = container.ChecksumError("block", 17)
    assert e.index == 17 and e.kind == "block" and "block 17" in str(e)


def test_command_line_takes_crc_and_no_verify():
    from cpprcoder_amd.__main__ import parser
    ap = parser()
    a = ap.parse_args(["c", "--crc", "-b", "4096", "in", "out"])
    assert a.crc and a.block == 4096 and (a.src, a.dst) == ("in", "out")
    assert not ap.parse_args(["c", "in", "out"]).crc
    a = ap.parse_args(["d", "--no-verify", "in", "out"])
    assert a.no_verify and not ap.parse_args(["d", "in", "out"]).no_verify
    a = ap.parse_args(["t", "--crc", "--coder", "rans8", "f1", "f2"])
    assert a.crc and a.files == ["f1", "f2"] and not ap.parse_args(["t", "f1"]).crc
    with pytest.raises(SystemExit):
        ap.parse_args(["d", "--crc", "in", "out"])


def test_library_exports_the_crc_calls():
    from cpprcoder_amd import build, rcx
    build.build()
    for name in CRC_SYMBOLS:
        assert name in rcx.EXPORTS and getattr(rcx.lib(), name) is not None
    assert len(rcx.EXPORTS) == 57 and rcx.lib().rcx_version() == 300
